"""encode.py --target-psnr / --target-bpsp end to end on the GPU, on the reference-made learnable 4 x 256 x 256 raster with
--target-k 3 6, -e 2, at -sr 1 and (one case) -sr 2.

No target is fixed in advance: a first run with a target every candidate meets (--target-psnr 0) logs the table, and the
targets of the other cases lie halfway between two neighbouring candidates of that table.  What a `Candidate` record states is
held to what the single runs produce: `bytes` to the size of the file `encode.main -K k` writes, `sse` to the exact sum
quality.compare finds between the decode of that file and the original.  The choice is lbdrn_hip.target.choose's on the logged
table, the chosen .bin is the single run's byte for byte, and no other candidate leaves a folder."""
import math
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from lbdrn_hip.target import Candidate, choose  # noqa: E402
from test_gpu_window_decode import _records, _settings  # noqa: E402

pytestmark = pytest.mark.gpu
KS = (3, 4, 5, 6)
COMMON = ["-e", "2", "-bs", "8192"]
RANGE = ["--target-k", "3", "6"]
CANDIDATE = re.compile(r"^Candidate K=(\d+): bytes=(\d+) bpsp=(\S+) sse=(\d+) mse=(\S+) psnr=(\S+)$")


def _sub(out, K=None):
    """the point folders under `out` (of one K, or all)"""
    if not os.path.isdir(out):
        return []
    return sorted(str(d) for d in out.iterdir() if d.is_dir() and (K is None or f"_K{K}_" in d.name))


def _table(records, n):
    """the `Candidate` records of a log as lbdrn_hip.target.Candidate, each held to its own figures"""
    out = []
    for r in records:
        m = CANDIDATE.match(r)
        if m:
            c = Candidate(int(m.group(1)), int(m.group(2)), int(m.group(4)), n)
            assert (float(m.group(3)), float(m.group(5)), float(m.group(6))) == (c.bpsp, c.mse, c.psnr()), r
            out.append(c)
    return out


def _strip(records, root):
    return [r.replace(str(root), "X") for r in records if not r.startswith("Time elapsed") and " fit " not in r]


class Runs:
    """the single runs (encode.main -K k, decode.main, quality.compare) of one split ratio, and the run that logs the table"""

    def __init__(self, work, img, sr):
        import decode
        import encode
        from lbdrn_hip import quality, raster_io
        self.work, self.img, self.sr, self.n = work, img, sr, img.size
        self.src = str(work / "scene.npy")
        np.save(self.src, img)
        self.args = ["-i", self.src, "-sr", str(sr)] + COMMON
        self.bin, self.records, self.sse = {}, {}, {}
        with _settings(None, "LBB2", None):
            for K in KS:
                out = work / f"single{K}"
                assert encode.main(self.args + ["-o", str(out), "-K", str(K)]) == 0
                (sub,) = _sub(out)
                binp = os.path.join(sub, "scene.bin")
                self.bin[K] = open(binp, "rb").read()
                self.records[K] = _strip(_records(os.path.join(sub, "encode.txt")), out)
                assert decode.main(["-i", binp]) == 0
                recon = raster_io.read_raster(binp[:-4] + "_recon.tif").reshape(img.shape)
                q = quality.compare(np.ascontiguousarray(recon), img)
                self.sse[K] = sum(b.sse for b in q.bands)
                assert self.sse[K] == int(((recon.astype(np.int64) - img.astype(np.int64)) ** 2).sum())
            self.first_status, self.first_out = self.target("first", ["--target-psnr", "0"])
        (sub,) = _sub(self.first_out)
        self.first_records = _records(os.path.join(sub, "encode.txt"))
        self.table = _table(self.first_records, self.n)

    def target(self, name, flags):
        import encode
        out = self.work / name
        with _settings(None, "LBB2", None):
            status = encode.main(self.args + ["-o", str(out)] + RANGE + flags)
        return status, out

    def check_chosen(self, out, want_K, target_text):
        """the run under `out` wrote the point want_K and nothing else, with the single run's bytes and records"""
        subs = _sub(out)
        assert subs == _sub(out, want_K) and len(subs) == 1, (subs, want_K)
        assert open(os.path.join(subs[0], "scene.bin"), "rb").read() == self.bin[want_K]
        assert sorted(os.listdir(subs[0])) == ["encode.txt", "scene.bin"]
        recs = _records(os.path.join(subs[0], "encode.txt"))
        assert _table(recs, self.n) == self.table                      # the same table, whatever the target
        assert [r for r in recs if r.startswith("Target")] == [f"Target: {target_text} -> K={want_K}"]
        rest = [r for r in _strip(recs, out) if not r.startswith(("Candidate K=", "Target"))]
        assert rest == self.records[want_K]
        assert recs[-1].startswith("Time elapsed")


@pytest.fixture(scope="module")
def runs(golden, dev, tmp_path_factory):
    img = np.ascontiguousarray(golden["rasters_learn_bands4"]["img"]).astype(np.uint16)
    assert img.shape == (4, 256, 256)
    return Runs(tmp_path_factory.mktemp("target_sr1"), img, 1)


def _halfway_targets(table):
    """(kind, value) halfway between neighbouring candidates, in PSNR and in bpsp"""
    by_psnr = sorted({c.psnr() for c in table if math.isfinite(c.psnr())})
    by_bpsp = sorted({c.bpsp for c in table})
    return [("psnr", (a + b) / 2) for a, b in zip(by_psnr, by_psnr[1:])] + [("bpsp", (a + b) / 2) for a, b in zip(by_bpsp, by_bpsp[1:])]


def test_the_table_is_what_the_single_runs_produce(runs):
    assert runs.first_status == 0
    assert [c.K for c in runs.table] == list(KS)                       # one record per candidate, in K order
    for c in runs.table:
        print(f"K={c.K}: bytes {c.nbytes} (file {len(runs.bin[c.K])}), sse {c.sse} (decode and compare {runs.sse[c.K]}), psnr {c.psnr()!r}")
        assert c.nbytes == len(runs.bin[c.K]) and c.sse == runs.sse[c.K]
    assert len({c.sse for c in runs.table}) == len(KS) and len(_halfway_targets(runs.table)) >= 4       # (there is something to choose)
    runs.check_chosen(runs.first_out, choose(runs.table, psnr=0.0).K, "psnr >= 0.0")


@pytest.mark.parametrize("kind,k", [(kind, k) for kind in ("psnr", "bpsp") for k in range(3)])
def test_a_target_between_two_candidates(runs, kind, k):
    targets = [t for t in _halfway_targets(runs.table) if t[0] == kind]
    if k >= len(targets):      # (two candidates of one size or one PSNR: fewer gaps than candidates - 1; the first test asserts >= 4 in all)
        k = len(targets) - 1
    value = targets[k][1]
    status, out = runs.target(f"{kind}{k}", [f"--target-{kind}", repr(value)])
    assert status == 0
    want = choose(runs.table, **{kind: value})
    runs.check_chosen(out, want.K, f"psnr >= {value}" if kind == "psnr" else f"bpsp <= {value}")
    if kind == "psnr":
        assert want.psnr() >= value and all(c.nbytes >= want.nbytes for c in runs.table if c.psnr() >= value)
    else:
        assert want.bpsp <= value and all(c.sse >= want.sse for c in runs.table if c.bpsp <= value)


@pytest.mark.parametrize("kind", ("psnr", "bpsp"))
def test_a_target_no_candidate_meets(runs, kind, capsys):
    value = max(c.psnr() for c in runs.table) + 1.0 if kind == "psnr" else min(c.bpsp for c in runs.table) / 2
    status, out = runs.target(f"unmet_{kind}", [f"--target-{kind}", repr(value), "-K", "9"])
    assert status == 3 and _sub(out) == [] and not any(f.endswith(".bin") for _, _, fs in os.walk(runs.work / f"unmet_{kind}") for f in fs)
    logged = [re.sub(r"^\[[^\]]*\] ", "", line) for line in capsys.readouterr().out.splitlines()]
    assert _table(logged, runs.n) == runs.table
    assert [r for r in logged if r.startswith("Target")] == [f"Target not met: {'psnr >=' if kind == 'psnr' else 'bpsp <='} {value}"]


def test_report_distortion_on_a_plain_encode(runs):
    import encode
    out = runs.work / "report"
    with _settings(None, "LBB2", None):
        assert encode.main(runs.args + ["-o", str(out), "-K", "5", "--report-distortion"]) == 0
    (sub,) = _sub(out)
    assert open(os.path.join(sub, "scene.bin"), "rb").read() == runs.bin[5]
    recs = _records(os.path.join(sub, "encode.txt"))
    c = Candidate(5, len(runs.bin[5]), runs.sse[5], runs.n)
    assert [r for r in recs if r.startswith("Closed-loop")] == [f"Closed-loop: sse={c.sse} mse={c.mse!r} psnr={c.psnr()!r}"]
    rest = [r for r in _strip(recs, out) if not r.startswith(("Closed-loop", "Namespace"))]
    assert rest == [r for r in runs.records[5] if not r.startswith("Namespace")]
    # beside a target: the record of the file that was written
    status, tout = runs.target("report_target", ["--target-psnr", "0", "--report-distortion"])
    (sub,) = _sub(tout)
    won = choose(runs.table, psnr=0.0)
    recs = _records(os.path.join(sub, "encode.txt"))
    assert status == 0 and [r for r in recs if r.startswith("Closed-loop")] == [f"Closed-loop: sse={won.sse} mse={won.mse!r} psnr={won.psnr()!r}"]


def test_four_tiles(golden, dev, tmp_path_factory):
    """-sr 2: both figures are sums over the tiles"""
    img = np.ascontiguousarray(golden["rasters_learn_bands4"]["img"]).astype(np.uint16)
    r = Runs(tmp_path_factory.mktemp("target_sr2"), img, 2)
    assert r.first_status == 0 and [c.K for c in r.table] == list(KS)
    for c in r.table:
        assert c.nbytes == len(r.bin[c.K]) and c.sse == r.sse[c.K]
    r.check_chosen(r.first_out, choose(r.table, psnr=0.0).K, "psnr >= 0.0")
    (kind, value) = _halfway_targets(r.table)[0]
    status, out = r.target("halfway", [f"--target-{kind}", repr(value)])
    assert status == 0
    r.check_chosen(out, choose(r.table, **{kind: value}).K, f"psnr >= {value}")
