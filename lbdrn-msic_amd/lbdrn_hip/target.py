"""Choose one of several encoded candidates by a PSNR or a size target (encode.py --target-psnr / --target-bpsp).

Host arithmetic only: a candidate is a K with the size of its file and its exact closed-loop sum of squared errors
(codec.closed_loop_sse), both sums over the tiles of the scene; nothing here touches a device."""
import collections
import math


class Candidate(collections.namedtuple("Candidate", "K nbytes sse n_samples")):
    """One point of the table.  nbytes: the whole .bin; sse: the integer sum over all samples of (original -
    reconstruction)^2; n_samples: bands x height x width."""
    __slots__ = ()

    @property
    def mse(self):
        return self.sse / self.n_samples

    def psnr(self, peak=10000.0):
        """10 log10(peak^2 / mse), the arithmetic of decode.py's `PSNR:` record; +inf for a lossless point"""
        return math.inf if self.sse == 0 else 10.0 * math.log10(peak ** 2 / self.mse)

    @property
    def bpsp(self):
        return self.nbytes * 8 / self.n_samples


class TargetNotMet(ValueError):
    """No candidate meets the target; `table` is the list of candidates that was searched."""

    def __init__(self, message, table):
        super().__init__(message)
        self.table = list(table)


def describe(psnr=None, bpsp=None):
    """the target as the records name it"""
    return f"psnr >= {psnr}" if psnr is not None else f"bpsp <= {bpsp}"


def choose(candidates, psnr=None, bpsp=None, peak=10000.0):
    """The candidate that meets the target at the least cost.

    psnr=P: among those with psnr(peak) >= P (sse == 0 counts as +inf) the smallest file; of equal files the larger K.
    bpsp=R: among those with bpsp <= R the smallest sse; of equal sse the smaller file.
    Exactly one of the two is given.  TargetNotMet (carrying the table) where nothing is eligible."""
    if (psnr is None) == (bpsp is None):
        raise ValueError("choose: exactly one of psnr and bpsp")
    table = list(candidates)
    if psnr is not None:
        ok = [c for c in table if c.psnr(peak) >= psnr]
        key = lambda c: (c.nbytes, -c.K)       # noqa: E731
    else:
        ok = [c for c in table if c.bpsp <= bpsp]
        key = lambda c: (c.sse, c.nbytes)      # noqa: E731
    if not ok:
        raise TargetNotMet(f"no candidate of K = {[c.K for c in table]} meets {describe(psnr, bpsp)}", table)
    return min(ok, key=key)
