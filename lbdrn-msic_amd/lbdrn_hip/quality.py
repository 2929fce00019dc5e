"""Two rasters compared on the GPU: the ctypes binding of liblbdrn_quality.so (include/lbdrn_quality.h, csrc/quality.hip,
csrc/quality.inc) -- exact per-band error statistics with the error histogram, SSIM per band in float64 and the spectral
angle (SAM) per pixel -- and the figures derived from them.  Built by csrc/build.py beside liblbdrn_tiffw.so;
LBDRN_QUALITY_LIB names another file.

    compare(a, b, peak=10000.0, ssim=True, sam=True, stream=None) -> Quality
        a, b: [C,H,W] or [H,W], uint8 or uint16, tensors in HBM (16-bit samples as int16 or uint16 storage; a view with unit
        innermost stride is compared where it lies) or numpy arrays (uploaded once).  One host sync: the result's download.
    Quality.bands[c], Quality.overall   the derived figures, float64 on the host
    Quality.to_records()                the log lines of decode.py --metrics
    Quality.to_json()                   everything, histograms included

    python -m lbdrn_hip.quality A B [--window X0 Y0 W H] [--peak P] [--json FILE]

The default peak is 10000, the fixed PSNR peak of decode.py's `PSNR:` record."""
import ctypes
import json
import math

import numpy as np

from ._native import E_ARG, E_DEVICE, E_UNSUPPORTED, E_WORKSPACE, Library, NativeError  # noqa: F401

ABI_VERSION = 1
SSIM, SAM = 1, 2                                                    # LBDRN_QUALITY_SSIM, LBDRN_QUALITY_SAM
HIST_BINS = 257
BAND_WORDS, PIXEL_WORDS = 5 + HIST_BINS + 2, 4                      # 8-byte fields of a band record and of the pixel record
DEFAULT_PEAK = 10000.0


class QualityError(NativeError):
    pass


_i32, _i64, _u32, _vp, _sz = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_size_t
SIGNATURES = {      # name -> (restype, argtypes): every function of include/lbdrn_quality.h
    "lbdrn_quality_last_error": (ctypes.c_char_p, []),
    "lbdrn_quality_abi_version": (ctypes.c_int, []),
    "lbdrn_quality_result_bytes": (_sz, [_i32]),
    "lbdrn_quality_workspace": (_sz, [_i32, _i32, _i32, _u32]),
    "lbdrn_quality_compare": (ctypes.c_int, [_vp, _i64, _i64, _vp, _i64, _i64, _i32, _i32, _i32, _i32, ctypes.c_double, _u32, _vp, _vp,
                                             _sz, _vp]),
}
_NATIVE = Library("liblbdrn_quality.so", "LBDRN_QUALITY_LIB", "lbdrn_quality_", ABI_VERSION, SIGNATURES, QualityError)
lib, available, _check, _PATH = _NATIVE.lib, _NATIVE.available, _NATIVE.check, _NATIVE.path


# ---------------------------------------------------------------- the result and what is derived from it

def _psnr(peak, mse):
    return math.inf if mse == 0 else 10.0 * math.log10(peak * peak / mse)


class Band:
    """One band: the raw integers (n, sse, sae, sum_err, max_abs, hist[257], ssim_n), ssim_sum, and the figures derived from
    them in float64."""

    def __init__(self, peak, n, sse, sae, sum_err, max_abs, hist, ssim_n, ssim_sum):
        self.n, self.sse, self.sae, self.sum_err, self.max_abs = int(n), int(sse), int(sae), int(sum_err), int(max_abs)
        self.hist = [int(v) for v in hist]
        self.ssim_n, self.ssim_sum = int(ssim_n), float(ssim_sum)
        self.mse = self.sse / self.n
        self.psnr = _psnr(peak, self.mse)
        self.mae = self.sae / self.n
        self.bias = self.sum_err / self.n
        self.ssim = self.ssim_sum / self.ssim_n if self.ssim_n else math.nan
        self.exact_share = self.hist[0] / self.n


class Overall:
    """The raster: sums over the bands, the mean of the bands' SSIM, and the spectral angle over the pixels."""

    def __init__(self, peak, bands, sam_n, sam_undefined, sam_sum, sam_max):
        n = sum(b.n for b in bands)
        self.n = n
        self.sse, self.sae = sum(b.sse for b in bands), sum(b.sae for b in bands)
        self.max_abs = max(b.max_abs for b in bands)
        self.mse = self.sse / n
        self.psnr = _psnr(peak, self.mse)
        self.mae = self.sae / n
        with_ssim = [b.ssim for b in bands if b.ssim_n]
        self.ssim = math.fsum(with_ssim) / len(with_ssim) if with_ssim else math.nan
        self.sam_n, self.sam_undefined = int(sam_n), int(sam_undefined)
        self.sam_sum, self.sam_max = float(sam_sum), float(sam_max)
        self.sam_mean = self.sam_sum / self.sam_n if self.sam_n else math.nan
        if not self.sam_n:
            self.sam_max = math.nan


def _num(v):
    """a float as the records and the JSON spell it: repr, so that it reads back to the same double"""
    return repr(float(v))


class Quality:
    def __init__(self, raw, C, peak, shape=None):
        """raw: the result of lbdrn_quality_compare as 264 C + 4 uint64 words"""
        raw = np.ascontiguousarray(raw, dtype=np.uint64)
        assert raw.size == C * BAND_WORDS + PIXEL_WORDS
        self.raw, self.peak, self.shape = raw, float(peak), shape
        self.bands = []
        for c in range(C):
            r = raw[c * BAND_WORDS:(c + 1) * BAND_WORDS]
            self.bands.append(Band(self.peak, r[0], r[1], r[2], r[3:4].view(np.int64)[0], r[4], r[5:5 + HIST_BINS], r[5 + HIST_BINS],
                                   r[6 + HIST_BINS:7 + HIST_BINS].view(np.float64)[0]))
        p = raw[C * BAND_WORDS:]
        self.overall = Overall(self.peak, self.bands, p[0], p[1], p[2:3].view(np.float64)[0], p[3:4].view(np.float64)[0])

    def to_records(self):
        """one line per band and one for the raster; none of them holds a pattern results_summary.py scrapes"""
        out = []
        for c, b in enumerate(self.bands):
            out.append(f"Quality band {c}: mse={_num(b.mse)} psnr={_num(b.psnr)} mae={_num(b.mae)} max={b.max_abs} bias={_num(b.bias)} "
                       f"exact={_num(b.exact_share)} ssim={_num(b.ssim)}")
        o = self.overall
        out.append(f"Quality: mse={_num(o.mse)} psnr={_num(o.psnr)} mae={_num(o.mae)} max={o.max_abs} ssim={_num(o.ssim)} "
                   f"sam_deg={_num(math.degrees(o.sam_mean))} sam_max_deg={_num(math.degrees(o.sam_max))}")
        return out

    def to_dict(self):
        def f(v):      # JSON has no inf / nan: they go as strings that float() reads back
            return v if math.isfinite(v) else repr(v)
        o = self.overall
        return {
            "peak": self.peak, "shape": list(self.shape) if self.shape is not None else None,
            "bands": [{"n": b.n, "sse": b.sse, "sae": b.sae, "sum_err": b.sum_err, "max_abs": b.max_abs, "hist": b.hist,
                       "ssim_n": b.ssim_n, "ssim_sum": b.ssim_sum, "mse": b.mse, "psnr": f(b.psnr), "mae": b.mae, "bias": b.bias,
                       "exact_share": b.exact_share, "ssim": f(b.ssim)} for b in self.bands],
            "overall": {"n": o.n, "sse": o.sse, "sae": o.sae, "max_abs": o.max_abs, "mse": o.mse, "psnr": f(o.psnr), "mae": o.mae,
                        "ssim": f(o.ssim), "sam_n": o.sam_n, "sam_undefined": o.sam_undefined, "sam_sum": o.sam_sum,
                        "sam_mean": f(o.sam_mean), "sam_max": f(o.sam_max)},
        }

    def to_json(self):
        return json.dumps(self.to_dict())


def parse_record(line):
    """a line of to_records() -> (band index or None, {name: value}); integers as int, the rest as float"""
    head, _, rest = line.partition(": ")
    band = int(head[len("Quality band "):]) if head.startswith("Quality band ") else None
    if band is None and head != "Quality":
        raise ValueError(f"not a quality record: {line!r}")
    vals = {}
    for item in rest.split():
        k, _, v = item.partition("=")
        vals[k] = int(v) if k == "max" else float(v)
    return band, vals


# ---------------------------------------------------------------- the call

def _describe(x):
    """(shape as (C, H, W), bits) of an argument, or ValueError; needs no device"""
    import torch
    if isinstance(x, torch.Tensor):
        bits = {torch.uint8: 8, torch.int16: 16, torch.uint16: 16}.get(x.dtype)
    elif isinstance(x, np.ndarray):
        bits = {np.uint8: 8, np.uint16: 16}.get(x.dtype.type)
    else:
        raise ValueError(f"{type(x).__name__}: a tensor in HBM or a numpy array is compared")
    if bits is None:
        raise ValueError(f"{x.dtype} samples: uint8 and uint16 rasters are compared")
    if x.ndim not in (2, 3):
        raise ValueError(f"shape {tuple(x.shape)}: [C,H,W] or [H,W]")
    shape = tuple(int(v) for v in x.shape)
    return ((1,) + shape if len(shape) == 2 else shape), bits


def _on_device(x, dev):
    import torch
    from . import ops
    if isinstance(x, np.ndarray):
        t = ops.to_device_u16(x, dev) if x.dtype == np.uint16 else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    else:
        t = x
    if t.dim() == 2:
        t = t[None]
    if t.stride(2) != 1 or t.stride(1) < t.shape[2] or t.stride(0) < 0:      # (the strides the library takes)
        t = t.contiguous()
    return t


def compare(a, b, peak=DEFAULT_PEAK, ssim=True, sam=True, stream=None):
    import torch
    (sa, ba), (sb, bb) = _describe(a), _describe(b)
    if sa != sb:
        raise ValueError(f"the rasters differ in shape: {sa} and {sb}")
    if ba != bb:
        raise ValueError(f"the rasters differ in sample type: {ba}-bit and {bb}-bit")
    if min(sa) < 1:
        raise ValueError(f"an empty raster: {sa}")
    if not (peak > 0 and math.isfinite(peak)):
        raise ValueError(f"peak = {peak}: a positive finite number")
    devs = [x.device for x in (a, b) if isinstance(x, torch.Tensor)]
    if any(d.type != "cuda" for d in devs) or len(set(devs)) > 1:
        raise ValueError("tensors are compared where they lie, in the HBM of one device; pass host data as numpy arrays")
    C, H, W = sa
    what = (SSIM if ssim else 0) | (SAM if sam else 0)
    L = lib()
    nres, nws = L.lbdrn_quality_result_bytes(C), L.lbdrn_quality_workspace(C, H, W, what)
    if not nres or (H * W > 1 << 31) or H > 1 << 20 or W > 1 << 20:
        raise ValueError(f"geometry {C} x {H} x {W} is out of the library's range")
    if not devs and not torch.cuda.is_available():
        raise QualityError("rasters are compared on the GPU; there is no CPU path in this package")
    dev = devs[0] if devs else torch.device("cuda:0")
    with torch.cuda.device(dev):
        s = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(s):
            ta, tb = _on_device(a, dev), _on_device(b, dev)
            result = torch.empty(nres // 8, dtype=torch.int64, device=dev)
            ws = torch.empty(max(nws, 8) // 8, dtype=torch.int64, device=dev)
            _check(L.lbdrn_quality_compare(ta.data_ptr(), ta.stride(1), ta.stride(0), tb.data_ptr(), tb.stride(1), tb.stride(0), ba,
                                           C, H, W, float(peak), what, result.data_ptr(), ws.data_ptr(), nws, s.cuda_stream),
                   "lbdrn_quality_compare")
            raw = result.cpu().numpy().view(np.uint64)      # the one host sync
    return Quality(raw, C, peak, shape=sa)


# ---------------------------------------------------------------- the command line

def main(argv=None):
    import argparse
    import sys
    p = argparse.ArgumentParser(prog="python -m lbdrn_hip.quality", description="compare two rasters on the GPU")
    p.add_argument("a")
    p.add_argument("b")
    p.add_argument("--window", type=int, nargs=4, default=None, metavar=("X0", "Y0", "W", "H"), help="compare this part only")
    p.add_argument("--peak", type=float, default=DEFAULT_PEAK, help="the peak of PSNR and SSIM (default 10000)")
    p.add_argument("--json", type=str, default=None, metavar="FILE", help="write every figure, histograms included")
    args = p.parse_args(argv)
    from . import raster_io
    if args.window is not None:      # checked against both rasters' sizes before a pixel is read, then only the windows are
        x0, y0, w, h = args.window
        for name in (args.a, args.b):
            _, H, W, _ = raster_io.raster_shape(name)
            if w < 1 or h < 1 or x0 < 0 or y0 < 0 or x0 + w > W or y0 + h > H:
                print(f"--window {x0} {y0} {w} {h} is not inside {name} ({W} x {H})", file=sys.stderr)
                return 2
        ta, tb = (raster_io.read_raster_device(name, window=(x0, y0, w, h)) for name in (args.a, args.b))
    else:
        ta, tb = raster_io.read_raster_device(args.a), raster_io.read_raster_device(args.b)
    try:
        q = compare(ta, tb, peak=args.peak)
    except ValueError as e:
        print(f"{args.a} and {args.b}: {e}", file=sys.stderr)
        return 2
    for line in q.to_records():
        print(line)
    if args.json is not None:
        with open(args.json, "w") as f:
            f.write(q.to_json())
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
