"""LBDRN-MSIC encoder, MI355X build: same command line, output directory naming, .bin container
and log records as the reference's encode.py (ref encode.py:167-289); the per-image fit runs as
fused HIP kernels (lbdrn_hip.codec.fit_image) instead of DataLoader + ignite + autograd.

Bitstream: header | for each tile (row-major): network payload | MSB payload   (ref encode.py:29-36)
           [| residual-layer trailer, with --max-error T: container.pack_residual_trailer]
           [| nodata chunk, with --nodata V: container.pack_nodata_trailer (lbdrn_hip/nodata.py)]
           [| geo-tag chunk, with --keep-tags on a source that has tags: container.pack_geo_trailer]

Multi-GPU: `python -m torch.distributed.run --nproc-per-node N encode.py ... -sr S` fits the S*S tiles of the
image round-robin on N GPUs (one process per GPU, no exchange during the fits) and rank 0 assembles the
.bin; the result is byte-identical to the single-GPU run because every rank replays the random draws of
the tiles it does not fit (lbdrn_hip.codec.skip_fit_rng).
"""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

import logger
from lbdrn_hip import codec, container, geotags, nodata, raster_io, sampler, shard
from lbdrn_hip.features import FeatCfg
from LBDRNdataset import tile_windows

DEVICE = "cuda:0"
BASE_CODEC = os.environ.get("LBDRN_BASE_CODEC", "LBB2")   # "jp2": JPEG 2000 through OpenJPEG, what the reference writes;
                                                          # "jp2-gpu": the same format coded on the GPU (csrc/jp2k.hip)
                                                          # (encode.py:137); "LBB1": the portable host payload of older files;
                                                          # "LBB3": LBB2 with inter-band prediction (csrc/plane3.hip)
REPORT_BOTH = os.environ.get("LBDRN_REPORT_BOTH_BPSP", "") not in ("", "0")   # also log the size of the payload format NOT
# written (JPEG 2000 costs 2-3 s of one host core per 8 x 2048^2 tile: off by default)
IN_FLIGHT = int(os.environ["LBDRN_IN_FLIGHT"]) if "LBDRN_IN_FLIGHT" in os.environ else None   # tiles of one image
# progressing at a time on a GPU (None: codec.fit_many's default, 4)


def tile_reads_wanted():
    """LBDRN_TILE_READS=1: at -sr > 1 read each tile as a window of the scene (raster_io.read_raster(window=)), the next
    one on a host thread, and never hold the scene; off by default.  Looked up when a run starts."""
    return os.environ.get("LBDRN_TILE_READS", "") not in ("", "0")


def write_image_header(header_path, split_ratio, width, height, K, bc, nl, D, nn_bytes_list,
                       base_bytes_list):
    data = container.pack_header(split_ratio, width, height, K, bc, nl, D, nn_bytes_list, base_bytes_list)
    with open(header_path, "wb") as f:
        f.write(data)
    if os.path.getsize(header_path) != data[0]:
        raise ValueError(f"Invalid number of bytes in header! expected {data[0]}, "
                         f"got {os.path.getsize(header_path)}")


def train(args, img=None):
    """Fit one image or tile and return (nn_payload, base_payload); logs what the reference logs
    (ref encode.py:67-157)."""
    if img is None:
        img = raster_io.read_raster(args.path)
    res = codec.fit_image(img, args.K, args.D, args.base_channel, args.num_layers, args.lr,
                          args.batch_size, args.epochs, args.val_duration,
                          cfg=FeatCfg.from_constants(), device=DEVICE, host_msb=False, nodata=fit_nodata(args))
    return report_and_pack(args, res)


class BasePayloadsAhead:
    """The JPEG 2000 MSB payloads of an image's tiles, coded WHILE the GPU fits (round 6).  The MSB planes are `tile >> K`
    (ref LBDRNdataset.py:95): known the moment the raster is read, long before the fit ends -- and the reference's own format
    (LBDRN_BASE_CODEC=jp2: what `gdal_translate -of JP2OpenJPEG` writes, ref encode.py:137) costs 0.8-1.3 s of eight host
    threads per 8 x 2048^2 tile against a 0.1 s fit.  One background thread codes the tiles in order, OpenJPEG's own worker
    threads inside each call (lbdrn_jp2_set_threads; the ctypes call releases the interpreter); report_and_pack takes the
    finished payload -- the same bytes as coding it afterwards -- or waits for it."""

    def __init__(self, tiles, K):
        import threading
        self.payloads, self.errors, self.seconds = {}, {}, {}
        self._done = {k: threading.Event() for k in range(len(tiles))}

        def work():
            for k, tile in enumerate(tiles):
                t0 = time.time()
                try:
                    msb = np.asarray(tile).reshape((-1,) + tile.shape[-2:]) >> K
                    msb = msb.astype(np.uint8) if int(msb.max()) <= 255 else msb.astype(np.uint16)      # LBDRNdataset.py:100
                    self.payloads[k] = container.encode_base(msb, codec="jp2")
                except Exception as e:   # (reported where the payload is asked for)
                    self.errors[k] = e
                self.seconds[k] = time.time() - t0
                self._done[k].set()
        self._thread = threading.Thread(target=work, name="lbdrn-jp2-ahead", daemon=True)
        self._thread.start()

    def take(self, k):
        self._done[k].wait()
        if k in self.errors:
            raise self.errors[k]
        return self.payloads.pop(k)


def report_and_pack(args, res, base_ahead=None):
    """The records train() logs for one finished fit, and its two payloads.  base_ahead: () -> the MSB payload coded meanwhile."""
    filename = os.path.splitext(os.path.basename(args.path))[0]
    logger.log.info("total_params: {}".format(res.params.size))
    for epoch, mse, improved in res.epoch_mse:
        if improved:
            logger.log.info("Save current best val model (MSE: {:.5f}) @epoch {}".format(mse, epoch))
        else:
            logger.log.info("Model is not updated (MSE: {:.5f}) @epoch: {}".format(mse, epoch))
    logger.log.info("best epoch: {}".format(res.best_epoch))
    nn_payload = container.encode_weights(res.params, args.precision)      # ref encode.py:129
    logger.log.info(f"nn: {len(nn_payload)} bytes, bpsp={len(nn_payload) * 8 / res.n_subpixels}")
    # ref encode.py:137 (gdal_translate to JP2): here the plane is coded where the fit left it, in HBM;
    # uint8 when it fits, like the reference's MSB raster (LBDRNdataset.py:100)
    if base_ahead is not None:
        t0 = time.time()
        base_payload = base_ahead()
        logger.log.info(f"MSB payload ({BASE_CODEC}) coded beside the fit; waited {time.time() - t0:.3f}s more for it")
    elif BASE_CODEC in ("LBB2", "LBB3") or BASE_CODEC.lower() == container.JP2_GPU_CODEC:   # coded from the plane in HBM
        base_payload = container.encode_base(res.msb_device, codec=BASE_CODEC, device=DEVICE, as_uint8=res.msb_max <= 255)
    else:
        base_payload = container.encode_base(_host_msb(res), codec=BASE_CODEC)
    logger.log.info(f"MSB: {len(base_payload)} bytes: bpsp={len(base_payload) * 8 / res.n_subpixels}")
    if REPORT_BOTH:   # the other payload's size beside the one written: LBB2 is this package's private format, jp2 the
        # reference's (the bpsp the published tables are in); the record does not match results_summary.py's patterns
        other = "jp2" if BASE_CODEC == "LBB2" else "LBB2"
        try:
            alt = (container.encode_base(_host_msb(res), codec="jp2") if other == "jp2" else
                   container.encode_base(res.msb_device, device=DEVICE, as_uint8=res.msb_max <= 255))
            logger.log.info(f"MSB as {other}: {len(alt)} bytes: bpsp={len(alt) * 8 / res.n_subpixels} (written: {BASE_CODEC})")
        except Exception as e:   # (liblbdrn_jp2.so absent: say so, the run goes on)
            logger.log.info(f"MSB as {other}: unavailable ({e})")
    logger.log.info(f"{filename}: fit {res.seconds['fit']:.3f}s on {DEVICE}")
    return nn_payload, base_payload


def residual_layer(args, res, tile, nn_payload, mask=None):
    """--max-error T: the tile's residual layer, coded in a closed loop against what the decoder will reconstruct from
    `nn_payload` and verified before it is handed back (lbdrn_hip.codec.residual_encode) -> LBR1 body.  mask: the tile's
    (kind, body, count) under --nodata; the loop then runs through the mask step and T bounds the chain's result."""
    more = {} if mask is None else {"nodata": (args.nodata, mask[0], mask[1])}
    body, err = codec.residual_encode(res, args.max_error, tile, nn_payload, args.K, args.D, args.base_channel, args.num_layers,
                                      cfg=FeatCfg.from_constants(), device=DEVICE, **more)
    logger.log.info(f"Max error: {err}")
    logger.log.info(f"Residual layer: {len(body)} bytes: bpsp={len(body) * 8 / res.n_subpixels}")
    return body


def nodata_value(parser, args):
    """--nodata V | tag -> args.nodata as the sample value (the attribute is absent without the flag, like `window`), before
    anything is read, fitted or written: a number outside 0..65535, or `tag` on a scene whose GDAL_NODATA is missing or
    names no integer sample value, ends the run here."""
    text = getattr(args, "nodata", None)
    if text is None:
        return None
    if str(text).strip().lower() == "tag":
        V = geotags.stored_nodata(raster_io.read_geo_tags(args.path), 16)
        if V is None:
            parser.error(f"--nodata tag: {args.path} has no GDAL_NODATA tag that names an integer sample value (0..65535)")
    else:
        try:
            V = nodata.check_value(int(str(text).strip()))
        except ValueError:
            parser.error(f"--nodata {text}: a sample value (0..65535), or `tag` for the scene's GDAL_NODATA")
    args.nodata = V
    return V


def nodata_fit_mode(parser, args):
    """--nodata-fit {all,valid}: `valid` fits and ranks on the valid pixels only and needs --nodata, which names the value.
    (Both attributes are absent without their flags, like `window`: the records of such a run stay.)"""
    mode = getattr(args, "nodata_fit", None)
    if mode == "valid" and getattr(args, "nodata", None) is None:
        parser.error("--nodata-fit valid needs --nodata V|tag: it names the value that marks a pixel as not to be fitted")
    return mode


def fit_nodata(args):
    """what the fit functions get as `nodata`: V under --nodata-fit valid, else None (the fit steps every pixel)"""
    return args.nodata if getattr(args, "nodata_fit", None) == "valid" else None


def nodata_fit_record(n_valid, n_pixels, batch_size):
    """the record --nodata-fit valid adds per tile"""
    return f"Nodata fit: {n_valid} of {n_pixels} pixels, {sampler.steps_per_epoch(n_valid, batch_size)} steps per epoch"


def report_nodata_fit(args, res, tile):
    if fit_nodata(args) is not None:
        logger.log.info(nodata_fit_record(res.n_valid, tile.shape[-2] * tile.shape[-1], args.batch_size))


def nodata_mask(args, tile):
    """--nodata V: the tile's entry of the nodata chunk, formed on the device from the tile's planes -> (kind, body, count)
    (lbdrn_hip.nodata.tile_mask).  It does not depend on K."""
    from lbdrn_hip import ops
    return nodata.tile_mask(ops.to_device_u16(codec._as_planes(tile), DEVICE), args.nodata)


def nodata_layer(args, res, tile, nn_payload, mask):
    """What --nodata adds to one tile behind report_and_pack: the residual layer through the mask step (with --max-error), or
    the chain check alone (without); then the tile's `Nodata:` record -> the LBR1 body or None."""
    if args.max_error is not None:
        layer = residual_layer(args, res, tile, nn_payload, mask)
    else:
        layer = None
        codec.nodata_verify(res, (args.nodata, mask[0], mask[1]), tile, nn_payload, args.K, args.D, args.base_channel,
                            args.num_layers, cfg=FeatCfg.from_constants(), device=DEVICE)
    logger.log.info(f"Nodata: V={args.nodata}, {mask[2]} samples, mask {len(mask[1])} bytes")
    return layer


def nodata_chunk(args, masks):
    """the 'LBNT' chunk of a file's tiles (masks: (kind, body, count) in tile order) and the file's `Nodata:` record"""
    chunk = container.pack_nodata_trailer(args.nodata, [(kind, body) for kind, body, _ in masks])
    return chunk, f"Nodata: V={args.nodata}, {sum(m[2] for m in masks)} samples, mask {len(chunk)} bytes"


def layer_tau(args):
    """what the 'LBRT' trailer stores: T, or with --nodata the bound the bodies were quantised for (nodata.tau_for)"""
    V = getattr(args, "nodata", None)
    return args.max_error if V is None else nodata.tau_for(args.max_error, V)


def train_tiles(args, tiles, draws):
    """Several tiles of one image: fitted with IN_FLIGHT of them progressing at a time (their random draws
    were made beforehand, in tile order), then reported one after another like train() would.
    tiles: [(path, array)]; returns [(nn_payload, base_payload, log records or None)]."""
    results = codec.fit_images([arr for _, arr in tiles], args.K, args.D, args.base_channel, args.num_layers,
                               args.lr, args.batch_size, args.epochs, args.val_duration,
                               cfg=FeatCfg.from_constants(), device=DEVICE, host_msb=False, draws=draws,
                               in_flight=IN_FLIGHT, nodata=fit_nodata(args))
    return results


def train_tiles_at(args, arrays, Ks, draws):
    """train_tiles for fits that each bring their K (main_k_points: the tiles of one image at several K; an array or a
    FitDraws that serves several entries is the same object in every one of them) -> one result per entry, or the
    exception that fit ended with."""
    return codec.fit_images(arrays, Ks, args.D, args.base_channel, args.num_layers, args.lr, args.batch_size, args.epochs,
                            args.val_duration, cfg=FeatCfg.from_constants(), device=DEVICE, host_msb=False, draws=draws,
                            in_flight=IN_FLIGHT, errors="return", nodata=fit_nodata(args))


def _host_msb(res):
    from lbdrn_hip import ops
    msb = ops.from_device_u16(res.msb_device)
    return msb.astype(np.uint8) if res.msb_max <= 255 else msb


def build_parser():
    p = argparse.ArgumentParser(description="LBDRN-MSIC")
    p.add_argument("--seed", type=int, default=19920517)
    p.add_argument("-rn", "--randomness", action="store_true", help="Allow randomness during training?")
    p.add_argument("-i", "--path", type=str, help="path of input tif or img file")
    p.add_argument("-o", "--output_dir", default="outputs", type=str, help="output dir")
    p.add_argument("-sr", "--split_ratio", type=int, default=1, help="tile size (default: 1)")
    p.add_argument("-K", "--K", type=int, default=5, help=" (default: 5)")
    p.add_argument("-bc", "--base_channel", type=int, default=64, help="base channel (default: 64)")
    p.add_argument("-nl", "--num_layers", type=int, default=2, help="Number of layers (default: 2)")
    p.add_argument("-D", "--D", type=int, default=2, help="#neighbors (2D+1)^2")
    p.add_argument("-prec", "--precision", type=int, default=16, help=" (default: 16)")
    p.add_argument("-lr", "--lr", type=float, default=1e-3, help="learning rate (default: 1e-3)")
    p.add_argument("-bs", "--batch_size", type=int, default=8192, help="batch size (default: 8192)")
    p.add_argument("-e", "--epochs", type=int, default=10, help="number of epochs to train (default: 10)")
    p.add_argument("-vd", "--val_duration", type=int, default=1,
                   help="number of epoch duration for val (default: 1)")
    p.add_argument("--window", type=int, nargs=4, default=argparse.SUPPRESS, metavar=("X0", "Y0", "W", "H"),
                   help="encode this part of the scene only (scene pixels); the output is named <name>_x{X0}_y{Y0}_w{W}_h{H}")
    p.add_argument("--max-error", dest="max_error", type=int, default=None, metavar="T",
                   help="append a residual layer that bounds |original - reconstruction| by T on every sample (0: lossless); "
                        "default: no layer")
    p.add_argument("--keep-tags", dest="keep_tags", action="store_true", default=argparse.SUPPRESS,
                   help="carry the input's georeferencing and nodata tags in the .bin (moved to the window with --window): "
                        "decode.py puts them on its raster.  Default: the file the reference's reader expects, nothing behind it")
    p.add_argument("--nodata", dest="nodata", type=str, default=argparse.SUPPRESS, metavar="V|tag",
                   help="keep samples of this value exact: the decoded raster equals V exactly where the input does, whatever K "
                        "and --max-error are (tag: the input's integer GDAL_NODATA).  Appends a losslessly coded mask to the .bin")
    p.add_argument("--nodata-fit", dest="nodata_fit", choices=("all", "valid"), default=argparse.SUPPRESS,
                   help="with --nodata: `valid` trains and ranks the epochs on the valid pixels only (a pixel is void where all its "
                        "bands equal V); `all` (default) fits every pixel.  The .bin format is the same either way")
    # (absent from the namespace without their flags, like `window`: the records of a run without them stay what they were)
    goal = p.add_mutually_exclusive_group()
    goal.add_argument("--target-psnr", dest="target_psnr", type=float, default=argparse.SUPPRESS, metavar="P",
                      help="fit the K of --target-k side by side and write the smallest file whose closed-loop PSNR is at least P dB")
    goal.add_argument("--target-bpsp", dest="target_bpsp", type=float, default=argparse.SUPPRESS, metavar="R",
                      help="likewise, the file of least closed-loop distortion among those of at most R bits per sample")
    p.add_argument("--target-k", dest="target_k", type=int, nargs=2, default=argparse.SUPPRESS, metavar=("LO", "HI"),
                   help="with a target: the candidates K = LO..HI (default 1 8; within 1..11)")
    p.add_argument("--target-peak", dest="target_peak", type=float, default=argparse.SUPPRESS, metavar="P",
                   help="the peak of the closed-loop PSNR (default 10000, decode.py's `PSNR:` record)")
    p.add_argument("--report-distortion", dest="report_distortion", action="store_true", default=argparse.SUPPRESS,
                   help="log the exact closed-loop distortion of the file being written (one `Closed-loop:` record)")
    return p


TARGET_ARGS = ("target_psnr", "target_bpsp", "target_k", "target_peak")


def target_request(parser, args, sharded=False):
    """--target-psnr / --target-bpsp and what goes with them, checked before anything is read, fitted or written ->
    None, or (psnr or None, bpsp or None, [candidate K], peak).  Out of scope, a parser error each: a target or
    --report-distortion beside --max-error (a different quality contract) or --nodata (the mask step moves samples that
    decode to V, which the evaluation pass does not see), and a target under a tile-sharded launch."""
    psnr, bpsp = getattr(args, "target_psnr", None), getattr(args, "target_bpsp", None)
    wanted = psnr is not None or bpsp is not None
    report = getattr(args, "report_distortion", False)
    if hasattr(args, "target_k") and not wanted:
        parser.error("--target-k names the candidates of --target-psnr / --target-bpsp: it goes with one of them")
    if hasattr(args, "target_peak") and not (wanted or report):
        parser.error("--target-peak goes with --target-psnr, --target-bpsp or --report-distortion")
    lo, hi = getattr(args, "target_k", (1, 8))
    if not 1 <= lo <= hi <= 11:
        parser.error(f"--target-k {lo} {hi}: LO <= HI, both within 1..11")
    peak = getattr(args, "target_peak", 10000.0)
    if not peak > 0:
        parser.error(f"--target-peak {peak}: a positive sample value")
    for flag, on in (("a target", wanted), ("--report-distortion", report)):
        if on and args.max_error is not None:
            parser.error(f"{flag} does not go with --max-error: the residual layer is a quality contract of its own")
        if on and getattr(args, "nodata", None) is not None:
            parser.error(f"{flag} does not go with --nodata: the mask step moves samples the closed-loop sum does not see")
    if wanted and sharded:
        parser.error("a target does not go with a tile-sharded launch: its candidates are fitted side by side on one device")
    return (psnr, bpsp, list(range(lo, hi + 1)), peak) if wanted else None


def tile_distortion(args, res, tile, nn_payload):
    """the exact closed-loop SSE of one fitted tile (lbdrn_hip.codec.closed_loop_sse): an int"""
    return codec.closed_loop_sse(res, tile, nn_payload, args.K, args.D, args.base_channel, args.num_layers,
                                 cfg=FeatCfg.from_constants(), device=DEVICE)


def distortion_record(cand, peak):
    """--report-distortion's record for a whole file (cand: lbdrn_hip.target.Candidate)"""
    return f"Closed-loop: sse={cand.sse} mse={cand.mse!r} psnr={cand.psnr(peak)!r}"


def candidate_record(cand, peak):
    return (f"Candidate K={cand.K}: bytes={cand.nbytes} bpsp={cand.bpsp!r} sse={cand.sse} mse={cand.mse!r} "
            f"psnr={cand.psnr(peak)!r}")


def scene_tags(args, path, window):
    """--keep-tags: (the geo-tag chunk to append as the last thing of the .bin -- b"" for a source without tags: a .npy
    array, a TIFF that has none --, its `Tags:` record), else (b"", None).  With a window the tags are those of the crop
    (geotags.shift).  Reads the header, the IFD and the tags' values of the source, no pixel."""
    if not getattr(args, "keep_tags", False):      # (absent without the flag, like `window`: the records of such a run stay)
        return b"", None
    tags = raster_io.read_geo_tags(path)
    if window is not None:
        tags = geotags.shift(tags, window[0], window[1])
    if not tags:
        return b"", "Tags: none"
    chunk = container.pack_geo_trailer(tags)
    return chunk, f"Tags: {len(tags)} tags, {len(chunk)} bytes"


def scene_name(args):
    """the stem of everything main() writes: the input's, with --window the window behind it"""
    name = os.path.splitext(os.path.basename(args.path))[0]
    win = getattr(args, "window", None)
    return name if win is None else name + "_x{}_y{}_w{}_h{}".format(*win)


def check_scene_window(parser, args):
    """--window against the scene's size, before anything is read or written (codec.check_window's wording)"""
    if getattr(args, "window", None) is not None:
        try:
            C, H, W, _ = raster_io.raster_shape(args.path)
            args.window = list(codec.check_window(args.window, W, H))
        except ValueError as e:
            parser.error(f"--window: {e}")


def scene_geometry(path, window):
    """(C, height, width) of the scene to encode -- of the window where one is given -- without reading a pixel"""
    C, H, W, _ = raster_io.raster_shape(path)
    return (C, H, W) if window is None else (C, window[3], window[2])


def tiles_ahead(path, window, wins):
    """LBDRN_TILE_READS: the tiles `wins` (tile_windows entries) of the scene, or of its window, each read as a window of the
    file; tile k + 1 is read on a host thread while the caller prepares tile k.  Yields [C,h,w] arrays in order."""
    from concurrent.futures import ThreadPoolExecutor
    ox, oy = (0, 0) if window is None else window[:2]

    def read(win):
        _, _, x0, y0, w, h = win
        a = raster_io.read_raster(path, window=(ox + x0, oy + y0, w, h))
        return np.ascontiguousarray(a.reshape((-1,) + a.shape[-2:]))
    with ThreadPoolExecutor(1, thread_name_prefix="lbdrn-tile-read") as pool:
        nxt = pool.submit(read, wins[0]) if wins else None
        for k in range(len(wins)):
            cur = nxt.result()
            nxt = pool.submit(read, wins[k + 1]) if k + 1 < len(wins) else None
            yield cur


def main(argv=None, shard_tiles=None):
    """shard_tiles: spread the split_ratio tiles over the ranks of a torchrun launch (default: whenever
    WORLD_SIZE > 1; sweep.py passes False because it shards whole jobs instead)."""
    global DEVICE
    parser = build_parser()
    args = parser.parse_args(argv)
    if os.environ.get("LBDRN_WEIGHTS_CODEC") != "fpzip":
        try:   # a precision the payload coder refuses is refused here, not after the fit
            container.check_weight_precision(args.precision)
        except ValueError as e:
            parser.error(str(e))
    if args.max_error is not None and not 0 <= args.max_error <= 65535:
        parser.error(f"--max-error {args.max_error}: 0 (lossless) .. 65535")
    try:   # likewise an MSB payload codec nobody knows (LBDRN_BASE_CODEC)
        container.check_base_codec(BASE_CODEC)
    except ValueError as e:
        parser.error(str(e))
    if shard_tiles is None:
        shard_tiles = shard.env_world()[1] > 1
    target = target_request(parser, args, sharded=shard_tiles)
    check_scene_window(parser, args)
    window = getattr(args, "window", None)
    V = nodata_value(parser, args)
    nodata_fit_mode(parser, args)
    if target is not None:
        return main_target(args, target)
    report = getattr(args, "report_distortion", False)
    rank, world = 0, 1
    if shard_tiles:
        rank, world, local = shard.init_host_group()
        DEVICE = shard.bind_device(local)
    if not args.randomness:
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)
        random.seed(args.seed)
    org_path = args.path
    filename = scene_name(args)
    args.output_dir = "{}/{}_r{}_K{}_bc{}_nl{}_D{}_prec{}_lr{}_bs{}_e{}".format(
        args.output_dir, filename, args.split_ratio, args.K, args.base_channel, args.num_layers,
        args.D, args.precision, args.lr, args.batch_size, args.epochs)
    os.makedirs(args.output_dir, exist_ok=True)
    bitstream_path = f"{args.output_dir}/{filename}.bin"
    log_path = f"{args.output_dir}/encode.txt"
    done = False
    if os.path.exists(log_path) and os.path.exists(bitstream_path):
        with open(log_path) as f:
            done = "Time elapsed" in f.read()
    if world > 1:   # one decision for all ranks, taken before anyone touches the log file
        done = all(shard.all_to_all_objects(done))
    if done:
        if rank == 0:
            print("Bitstream already created!")
        if world > 1:
            shard.finish()
        return 0
    if rank == 0:
        logger.create_logger(args.output_dir, "encode.txt")
    else:
        logger.create_logger(args.output_dir, "", log_file_only=True)
    start_time = time.time()
    # --keep-tags: rank 0 alone opens the tags, before anything is fitted (a source they cannot be read from ends the run here)
    geo_chunk, geo_record = scene_tags(args, org_path, window) if rank == 0 else (b"", None)
    tile_reads = tile_reads_wanted() and args.split_ratio > 1
    if tile_reads:
        img = None
        C, height, width = scene_geometry(org_path, window)
    else:
        img = raster_io.read_raster(org_path) if window is None else raster_io.read_raster(org_path, window=window)
        img = img.reshape((-1,) + img.shape[-2:])
        C, height, width = img.shape
    windows = list(tile_windows(width, height, args.split_ratio)) if args.split_ratio > 1 else [None]
    n_feature = FeatCfg.from_constants().feature_dim(C, args.D)
    # every tile's random draws, in tile order, whoever fits it: the reference runs the tiles one after
    # another on one generator (ref encode.py:231-262)
    draws = [codec.draw_fit(n_feature, args.base_channel, C, args.num_layers, args.epochs, args.val_duration)
             for _ in windows]
    mine, jobs = [t for t in range(len(windows)) if t % world == rank], []
    ahead_tiles = tiles_ahead(org_path, window, [windows[t] for t in mine]) if tile_reads else None
    for t in mine:
        path, tile = org_path, img
        if windows[t] is not None:
            i, j, x0, y0, w, h = windows[t]
            path = f"{args.output_dir}/tile_{i}_{j}.tif"
            tile = next(ahead_tiles) if tile_reads else np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w])
        jobs.append((path, tile))
    # the reference's MSB format is host work that needs nothing from the fit: it starts now (LBDRN_JP2_AHEAD=0: afterwards, as before)
    ahead = None
    if jobs and BASE_CODEC.lower() in ("jp2", "jpeg2000", "jp2openjpeg") and os.environ.get("LBDRN_JP2_AHEAD", "1") != "0":
        ahead = BasePayloadsAhead([tile for _, tile in jobs], args.K)
    results = train_tiles(args, jobs, [draws[t] for t in mine]) if jobs else []
    fitted = []   # (tile index, nn payload, MSB payload, captured log records or None, residual body or None[, mask entry])
    sse = 0       # --report-distortion: the closed-loop sum of this rank's tiles
    for k, (t, (path, tile), res) in enumerate(zip(mine, jobs, results)):
        args.path = path
        take = (lambda k=k: ahead.take(k)) if ahead is not None else None
        mask = nodata_mask(args, tile) if V is not None else None
        if world > 1:
            with logger.capture() as lines:
                logger.log.info(args)
                nn, base = report_and_pack(args, res, take)
                report_nodata_fit(args, res, tile)
                layer = (nodata_layer(args, res, tile, nn, mask) if V is not None else
                         residual_layer(args, res, tile, nn) if args.max_error is not None else None)
        else:
            lines = None
            logger.log.info(args)
            nn, base = report_and_pack(args, res, take)
            report_nodata_fit(args, res, tile)
            layer = (nodata_layer(args, res, tile, nn, mask) if V is not None else
                     residual_layer(args, res, tile, nn) if args.max_error is not None else None)
        fitted.append((t, nn, base, lines, layer) + ((mask,) if V is not None else ()))      # the mask travels beside the layer
        if report:
            sse += tile_distortion(args, res, tile, nn)
    if report and world > 1:      # (exact integers: the order of the ranks' sums does not matter)
        sse = sum(shard.all_to_all_objects(sse))
    gathered = shard.gather_to_root(fitted) if world > 1 else [fitted]
    if rank == 0:
        tiles = sorted((rec for part in gathered for rec in part), key=lambda rec: rec[0])
        assert [rec[0] for rec in tiles] == list(range(len(windows)))
        for rec in tiles:
            if rec[3] is not None:
                logger.replay(rec[3])
        header = container.pack_header(args.split_ratio, width, height, args.K, args.base_channel,
                                       args.num_layers, args.D, [len(rec[1]) for rec in tiles],
                                       [len(rec[2]) for rec in tiles], activation=FeatCfg.from_constants().activation)
        with open(bitstream_path, "wb") as f:
            f.write(header)
            for rec in tiles:
                f.write(rec[1])
                f.write(rec[2])
            if args.max_error is not None:      # behind everything the header lists: older readers stop before it
                f.write(container.pack_residual_trailer(layer_tau(args), [rec[4] for rec in tiles]))
            if V is not None:                   # --nodata: between the layer and the tags
                chunk, nodata_record = nodata_chunk(args, [rec[5] for rec in tiles])
                f.write(chunk)
            f.write(geo_chunk)                  # --keep-tags: the last thing in the file, behind the layer where there is one
        if V is not None:
            logger.log.info(nodata_record)
        if geo_record is not None:
            logger.log.info(geo_record)
        if report:
            from lbdrn_hip.target import Candidate
            logger.log.info(distortion_record(Candidate(args.K, os.path.getsize(bitstream_path), sse, C * height * width),
                                              getattr(args, "target_peak", 10000.0)))
        logger.log.info(f"Time elapsed: {time.time() - start_time}")
    if world > 1:
        shard.finish()
    return 0


def output_folder(args):
    """The directory main() writes a point into (ref encode.py:207-209)."""
    filename = scene_name(args)
    return "{}/{}_r{}_K{}_bc{}_nl{}_D{}_prec{}_lr{}_bs{}_e{}".format(
        args.output_dir, filename, args.split_ratio, args.K, args.base_channel, args.num_layers,
        args.D, args.precision, args.lr, args.batch_size, args.epochs)


def main_target(base, target):
    """main() with --target-psnr P or --target-bpsp R: the candidates K of --target-k are fitted side by side as
    main_k_points fits them (the raster read and tiled once, one draw per tile, all (tile, K) fits through one
    codec.fit_many), every candidate's payloads are packed and its two figures taken for the whole scene -- the size of its
    file and its exact closed-loop SSE (tile_distortion), both sums over the tiles --, lbdrn_hip.target.choose picks one, and
    ONLY that point is written: into the folder main() with -K k names, the .bin byte for byte that run's, encode.txt that
    run's records (their times apart) plus one `Candidate` record per K and the `Target:` record.  Unchosen candidates leave
    nothing on disk.  Where no candidate meets the target the table and a `Target not met` record go to stdout, nothing is
    written, and the status is 3.  base: the parsed arguments (their -K is ignored); target: target_request's answer."""
    from lbdrn_hip.target import Candidate, TargetNotMet, choose, describe
    psnr, bpsp, Ks, peak = target
    plain = argparse.Namespace(**{k: v for k, v in vars(base).items() if k not in TARGET_ARGS})   # what `-K k` alone parses to
    window = getattr(base, "window", None)
    if not base.randomness:
        torch.manual_seed(base.seed)
        np.random.seed(base.seed)
        random.seed(base.seed)
    org_path = base.path
    filename = scene_name(base)
    start_time = time.time()
    geo_chunk, geo_record = scene_tags(base, org_path, window)
    tile_reads = tile_reads_wanted() and base.split_ratio > 1
    if tile_reads:
        img = None
        C, height, width = scene_geometry(org_path, window)
    else:
        img = raster_io.read_raster(org_path) if window is None else raster_io.read_raster(org_path, window=window)
        img = img.reshape((-1,) + img.shape[-2:])
        C, height, width = img.shape
    windows = list(tile_windows(width, height, base.split_ratio)) if base.split_ratio > 1 else [None]
    n_feature = FeatCfg.from_constants().feature_dim(C, base.D)
    draws = [codec.draw_fit(n_feature, base.base_channel, C, base.num_layers, base.epochs, base.val_duration)
             for _ in windows]      # one draw per tile, in tile order, serves every K
    tiles = []
    ahead_tiles = tiles_ahead(org_path, window, windows) if tile_reads else None
    for win in windows:
        tile = img
        if win is not None:
            i, j, x0, y0, w, h = win
            tile = next(ahead_tiles) if tile_reads else np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w])
        tiles.append(tile)
    ahead = {}
    if BASE_CODEC.lower() in ("jp2", "jpeg2000", "jp2openjpeg") and os.environ.get("LBDRN_JP2_AHEAD", "1") != "0":
        ahead = {K: BasePayloadsAhead(tiles, K) for K in Ks}
    entries = [(t, K) for t in range(len(tiles)) for K in Ks]      # tile-major: the K points of a tile are neighbours
    results = dict(zip(entries, train_tiles_at(base, [tiles[t] for t, _ in entries], [K for _, K in entries],
                                               [draws[t] for t, _ in entries])))
    # every candidate reported and packed as main() does it, its records kept aside until one of them is chosen
    logger.create_logger("", "")      # (stdout; no folder exists yet)
    table, packed = [], {}
    for K in Ks:
        a = argparse.Namespace(**vars(plain))
        a.K = K
        a.output_dir = output_folder(a)
        for t in range(len(tiles)):
            if isinstance(results[(t, K)], Exception):
                raise results[(t, K)]
        tiles_out, sse = [], 0
        with logger.capture() as lines:
            for t, (win, tile) in enumerate(zip(windows, tiles)):
                a.path = org_path if win is None else f"{a.output_dir}/tile_{win[0]}_{win[1]}.tif"
                take = (lambda t=t, K=K: ahead[K].take(t)) if K in ahead else None
                logger.log.info(a)
                nn, base_payload = report_and_pack(a, results[(t, K)], take)
                sse += tile_distortion(a, results[(t, K)], tile, nn)
                tiles_out.append((nn, base_payload))
        header = container.pack_header(a.split_ratio, width, height, K, a.base_channel, a.num_layers, a.D,
                                       [len(nn) for nn, _ in tiles_out], [len(b) for _, b in tiles_out],
                                       activation=FeatCfg.from_constants().activation)
        body = b"".join([header] + [part for rec in tiles_out for part in rec] + [geo_chunk])
        table.append(Candidate(K, len(body), sse, C * height * width))
        packed[K] = (a, lines, body)
    try:
        won = choose(table, psnr=psnr, bpsp=bpsp, peak=peak)
    except TargetNotMet:
        for cand in table:
            logger.log.info(candidate_record(cand, peak))
        logger.log.info(f"Target not met: {describe(psnr, bpsp)}")
        return 3
    a, lines, body = packed[won.K]
    os.makedirs(a.output_dir, exist_ok=True)
    logger.create_logger(a.output_dir, "encode.txt")
    logger.replay(lines)
    for cand in table:
        logger.log.info(candidate_record(cand, peak))
    logger.log.info(f"Target: {describe(psnr, bpsp)} -> K={won.K}")
    with open(f"{a.output_dir}/{filename}.bin", "wb") as f:
        f.write(body)
    if geo_record is not None:
        logger.log.info(geo_record)
    if getattr(base, "report_distortion", False):
        logger.log.info(distortion_record(won, peak))
    logger.log.info(f"Time elapsed: {time.time() - start_time}")
    return 0


def main_k_points(argv, Ks):
    """main() for several K of ONE raster, their fits side by side on the device: what `main(argv + ["-K", k])` for k in
    Ks writes, one after another -- the same directories, .bin bytes and encode.txt records (only the records' times
    differ: the `Time elapsed` record, the seconds of the `fit ...s on` record and of the jp2 `waited ...s more` one).
    Every point of a sweep re-seeds its generator (ref encode.py:200-205), so the K points of a raster have the same
    tiles, the same initial weights and the same minibatch orders: the raster is read and tiled once, the draws are made
    once per tile, and all (tile, K) fits go through one codec.fit_many, tile-major, so that the K points of a tile --
    one shape -- step in one launch per minibatch (codec.fit_group).  Then every K is reported and packed as main() does
    it.  One process, one GPU: the tiles are not spread over ranks (sweep.py deals whole points).  A -K in argv is
    ignored.  Returns {K: None, or the exception that point ended with}; a point that fails does not stop the others."""
    parser = build_parser()
    base = parser.parse_args(argv)
    Ks = [int(k) for k in Ks]
    if os.environ.get("LBDRN_WEIGHTS_CODEC") != "fpzip":
        try:
            container.check_weight_precision(base.precision)
        except ValueError as e:
            parser.error(str(e))
    if base.max_error is not None and not 0 <= base.max_error <= 65535:
        parser.error(f"--max-error {base.max_error}: 0 (lossless) .. 65535")
    try:
        container.check_base_codec(BASE_CODEC)
    except ValueError as e:
        parser.error(str(e))
    check_scene_window(parser, base)
    window = getattr(base, "window", None)
    V = nodata_value(parser, base)
    nodata_fit_mode(parser, base)
    if not base.randomness:
        torch.manual_seed(base.seed)
        np.random.seed(base.seed)
        random.seed(base.seed)
    org_path = base.path
    filename = scene_name(base)
    outcome, point, todo = {}, {}, []
    for K in Ks:
        a = argparse.Namespace(**vars(base))
        a.K = K
        a.output_dir = output_folder(a)
        os.makedirs(a.output_dir, exist_ok=True)
        point[K] = a
        bitstream_path, log_path = f"{a.output_dir}/{filename}.bin", f"{a.output_dir}/encode.txt"
        done = False
        if os.path.exists(log_path) and os.path.exists(bitstream_path):
            with open(log_path) as f:
                done = "Time elapsed" in f.read()
        if done:
            print("Bitstream already created!")
            outcome[K] = None
        else:
            todo.append(K)
    if not todo:
        return outcome
    start_time = time.time()
    try:
        geo_chunk, geo_record = scene_tags(base, org_path, window)      # --keep-tags: read once, carried by every K's file
        tile_reads = tile_reads_wanted() and base.split_ratio > 1
        if tile_reads:
            img = None
            C, height, width = scene_geometry(org_path, window)
        else:
            img = raster_io.read_raster(org_path) if window is None else raster_io.read_raster(org_path, window=window)
            img = img.reshape((-1,) + img.shape[-2:])
            C, height, width = img.shape
        windows = list(tile_windows(width, height, base.split_ratio)) if base.split_ratio > 1 else [None]
        n_feature = FeatCfg.from_constants().feature_dim(C, base.D)
        # one draw per tile, in tile order, serves every K (read-only: codec.fit_group)
        draws = [codec.draw_fit(n_feature, base.base_channel, C, base.num_layers, base.epochs, base.val_duration)
                 for _ in windows]
        tiles = []
        ahead_tiles = tiles_ahead(org_path, window, windows) if tile_reads else None
        for win in windows:
            tile = img
            if win is not None:
                i, j, x0, y0, w, h = win
                tile = next(ahead_tiles) if tile_reads else np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w])
            tiles.append(tile)
        ahead = {}
        if BASE_CODEC.lower() in ("jp2", "jpeg2000", "jp2openjpeg") and os.environ.get("LBDRN_JP2_AHEAD", "1") != "0":
            ahead = {K: BasePayloadsAhead(tiles, K) for K in todo}
        entries = [(t, K) for t in range(len(tiles)) for K in todo]      # tile-major: the K points of a tile are neighbours
        results = train_tiles_at(base, [tiles[t] for t, _ in entries], [K for _, K in entries], [draws[t] for t, _ in entries])
        results = dict(zip(entries, results))
    except Exception as e:      # nothing of this raster can be written: every open point ends with it
        for K in todo:
            outcome[K] = e
        return outcome
    shared_seconds = (time.time() - start_time) / len(todo)
    masks = {}      # --nodata: a tile's mask does not depend on K -- formed once, by the first point that gets there, shared by all
    for K in todo:
        a = point[K]
        t_point = time.time()
        try:
            for t in range(len(tiles)):
                if isinstance(results[(t, K)], Exception):
                    raise results[(t, K)]
            logger.create_logger(a.output_dir, "encode.txt")
            tiles_out = []
            for t, (win, tile) in enumerate(zip(windows, tiles)):
                a.path = org_path if win is None else f"{a.output_dir}/tile_{win[0]}_{win[1]}.tif"
                res = results[(t, K)]
                take = (lambda t=t, K=K: ahead[K].take(t)) if K in ahead else None
                logger.log.info(a)
                if V is not None and t not in masks:
                    masks[t] = nodata_mask(a, tile)
                nn, base_payload = report_and_pack(a, res, take)
                report_nodata_fit(a, res, tile)
                layer = (nodata_layer(a, res, tile, nn, masks[t]) if V is not None else
                         residual_layer(a, res, tile, nn) if a.max_error is not None else None)
                tiles_out.append((nn, base_payload, layer))
            header = container.pack_header(a.split_ratio, width, height, K, a.base_channel, a.num_layers, a.D,
                                           [len(rec[0]) for rec in tiles_out], [len(rec[1]) for rec in tiles_out],
                                           activation=FeatCfg.from_constants().activation)
            with open(f"{a.output_dir}/{filename}.bin", "wb") as f:
                f.write(header)
                for nn, base_payload, _ in tiles_out:
                    f.write(nn)
                    f.write(base_payload)
                if a.max_error is not None:
                    f.write(container.pack_residual_trailer(layer_tau(a), [rec[2] for rec in tiles_out]))
                if V is not None:
                    chunk, nodata_record = nodata_chunk(a, [masks[t] for t in range(len(tiles))])
                    f.write(chunk)
                f.write(geo_chunk)
            if V is not None:
                logger.log.info(nodata_record)
            if geo_record is not None:
                logger.log.info(geo_record)
            # this point's share of the reading and fitting all points did together, plus its own reporting and packing
            logger.log.info(f"Time elapsed: {shared_seconds + time.time() - t_point}")
            outcome[K] = None
        except Exception as e:
            outcome[K] = e
    return outcome


if __name__ == "__main__":
    sys.exit(main())
