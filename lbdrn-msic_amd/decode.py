"""LBDRN-MSIC decoder, MI355X build: same command line, log records and reconstruction as the
reference's decode.py (ref decode.py:151-224); feature rebuild, network forward, rounding and
integer reconstruction run as one fused HIP kernel (lbdrn_hip.codec.apply_image).

Under `python -m torch.distributed.run --nproc-per-node N decode.py ...` the split_ratio tiles of the
bitstream are decoded round-robin on N GPUs and merged on rank 0 (tiles are independent: no exchange
while decoding).

`--window X0 Y0 W H` reconstructs that part of the scene only (lbdrn_hip.codec.decode_window): tiles the window does not
touch are skipped by the byte sizes in the header, touched ones are decoded on a crop with a margin of D.

A file written with `encode.py --max-error T` carries a residual layer behind its payloads: it is applied by default (to a
window through the layer's rectangle argument: only the blocks the window touches are decoded); `--no-enhancement` gives the
base reconstruction.

`--out-compress deflate [--out-tile N]` writes the raster as a tiled, Deflate-compressed, predictor-2 TIFF
(raster_io.write_raster_device): at `-sr 1` and for a `--window` the reconstruction is compressed where it lies, in HBM, and only
the compressed bytes are downloaded; merged tiles and gathered ranks are uploaded once.  Without the flag nothing changes.
With it, `--out-overviews auto|N [--out-resampling average|nearest] [--out-nodata V]` adds overview levels, reduced on the GPU
from the reconstruction where it lies (lbdrn_hip.pyramid), and `--out-georef FILE` copies FILE's georeferencing tags onto the
output.  No log record changes.

A file written with `encode.py --keep-tags` carries the scene's georeferencing and nodata tags behind everything else
(container.unpack_geo_trailer): they go onto the output TIFF by default -- as stored for a whole decode, moved to the window's
origin for `--window` (lbdrn_hip.geotags.shift) -- with `--out-compress` through the same `geo=` option, without it through
raster_io.write_raster(path, image, geo=tags), and one record says so (`Tags: <n> tags restored`).  `--out-georef FILE` still
copies FILE's tags verbatim and wins; `--no-tags` ignores the chunk; a .npy output gets none.  With `--out-overviews` and no
`--out-nodata`, a stored GDAL_NODATA that is an integer sample value is the overviews' nodata.

A file written with `encode.py --nodata V` carries a losslessly coded mask of its nodata samples between those two
(container.unpack_nodata_trailer).  The mask step (lbdrn_hip.nodata.apply) is the last thing done to a tile's or a window
piece's reconstruction, in HBM: V where the mask is set, and a valid sample that decodes to V moves one count off it -- so the
raster equals V exactly where the original did.  One record says so (`Nodata: V=<V>`); `--no-mask` leaves the step out.  V is
the overviews' nodata with `--out-overviews` unless `--out-nodata` names one (it wins over a stored GDAL_NODATA), and a TIFF
output that gets no GDAL_NODATA from stored or copied tags gets one that names V.

`-org ORG --metrics [--metrics-peak P] [--metrics-json FILE]` adds, behind the `PSNR:` / `Max error:` record, one `Quality band c:`
line per band and one `Quality:` line for the raster (lbdrn_hip.quality.compare: error statistics, SSIM and the spectral angle,
computed on the GPU).  The other records are what they are without the flag."""
import argparse
import os
import random
import sys
import time

import numpy as np
import torch

import logger
from lbdrn_hip import codec, container, geotags, nodata, ops, raster_io, shard
from lbdrn_hip.features import FeatCfg
from LBDRNdataset import tile_windows, write_tiff_with_gdal

DEVICE = "cuda:0"
K = D = bc = nl = None  # set from the header; test() reads them like the reference's does
ACTIVATION = None       # "relu" / "sine" where the header names the hidden activation (container.header_activation), else None


def read_image_header(bitstream):
    return container.unpack_header(bitstream)


def test(bitstream, dirname, filename, nn_bytes, base_bytes, write=True, layer=None, out=None, geo=None, mask=None):
    """Decode one image or tile from the front of `bitstream`; returns the remaining bytes
    (ref decode.py:56-141).  layer: the tile's residual body (LBR1), applied to the reconstruction in HBM.  out: the
    options of --out-compress (raster_io.write_raster_device); the raster is then written from the reconstruction where it
    lies, without a host copy of it.  geo: the tags for a raster written without those options (write_plain).  mask: (V, kind,
    body) of the tile from the file's nodata chunk: the mask step, applied last, in HBM."""
    nn_payload, bitstream = bitstream[:nn_bytes], bitstream[nn_bytes:]
    base_payload, bitstream = bitstream[:base_bytes], bitstream[base_bytes:]
    base = container.decode_base(base_payload, device=DEVICE, keep_on_device=True)   # ref decode.py:69-73
    cfg = FeatCfg.from_constants()
    if ACTIVATION is not None and ACTIVATION != cfg.activation:   # the file says which network it holds: it wins over constants.py
        cfg.activation = ACTIVATION
    # the parameter count the header's network shape needs: a payload that holds another number is refused before
    # anything is sized by it (ref decode.py:114-120 slices the vector by state_dict shapes)
    need = ops.param_count(ops.make_net(cfg.feature_dim(int(base.shape[0]), D), bc, int(base.shape[0]), nl))
    params = container.decode_weights(nn_payload, expected=need)
    recon_path = f"{dirname}/{filename}_recon.tif"
    if write and out is not None:
        rec = codec.apply_image(base, params, K, D, bc, nl, cfg=cfg, device=DEVICE, keep_on_device=True)
        if layer is not None:
            rec = codec.residual_apply(layer, rec.contiguous())
        if mask is not None:
            rec = nodata.apply(rec.contiguous(), mask[1], mask[2], mask[0])
        raster_io.write_raster_device(recon_path, rec.contiguous(), **out)
        test.last_image = None
        logger.log.info(f"Recon: {recon_path}")
        return bitstream
    if layer is None and mask is None:
        image = codec.apply_image(base, params, K, D, bc, nl, cfg=cfg, device=DEVICE)
    else:
        rec = codec.apply_image(base, params, K, D, bc, nl, cfg=cfg, device=DEVICE, keep_on_device=True).contiguous()
        if layer is not None:
            rec = codec.residual_apply(layer, rec)
        if mask is not None:
            rec = nodata.apply(rec, mask[1], mask[2], mask[0])
        image = ops.from_device_u16(rec)
    test.last_image = image
    if write:
        write_plain(recon_path, image, geo)
        logger.log.info(f"Recon: {recon_path}")
    return bitstream


def write_plain(path, image, geo):
    """today's writer; with tags to restore, the same array through raster_io.write_raster(geo=): lbdrn_hip.tiff_write at
    compression "none" (GDAL's writer is never asked to carry them)"""
    if geo:
        raster_io.write_raster(path, image, geo=geo, device=DEVICE)
    else:
        write_tiff_with_gdal(path, image)


def stored_tags(args, bitstream, path, window=None):
    """The tags to put on the raster at `path` from the file's geo-tag chunk: as stored, or moved to the window's origin;
    None for a file without the chunk, under --no-tags, where --out-georef names the tags instead, and for a .npy output."""
    if args.no_tags:
        return None
    tags = container.unpack_geo_trailer(bitstream)
    if not tags or args.out_georef is not None or path.endswith(".npy"):
        return None
    return tags if window is None else geotags.shift(tags, window[0], window[1])


def stored_mask(args, bitstream):
    """(V, [(kind, body) per tile]) of a file with a nodata chunk (encode.py --nodata); None without one and under --no-mask"""
    return None if args.no_mask else container.unpack_nodata_trailer(bitstream)


def with_nodata_tag(tags, V, path):
    """`tags` (or None) with a GDAL_NODATA that names V added where they have none -- what a TIFF written from a masked
    reconstruction carries; unchanged without a mask (V None) and for a .npy output"""
    if V is None or path.endswith(".npy") or any(t[0] == geotags.GDAL_NODATA for t in tags or ()):
        return tags
    text = str(V).encode("ascii") + b"\0"
    return sorted(list(tags or []) + [(geotags.GDAL_NODATA, 2, len(text), text)], key=lambda t: t[0])


def out_options(args, geo=None, V=None, path=""):
    """the raster_io.write_raster_device options --out-compress / --out-tile / --out-overviews / --out-resampling / --out-nodata /
    --out-georef ask for; None: today's writer.  geo: the stored tags to restore (stored_tags): they ride the `geo` option,
    and their GDAL_NODATA, where it is an integer sample value, is the overviews' nodata unless --out-nodata names one.  V: the
    value of the file's nodata chunk where its mask is applied: it comes before the stored tag, and the tags written -- stored
    or copied -- get a GDAL_NODATA that names it where they have none (with_nodata_tag)."""
    if args.out_compress is None:
        return None
    out = {"compress": args.out_compress, "tile": args.out_tile}
    if args.out_overviews is not None:
        value = args.out_nodata if args.out_nodata is not None else V if V is not None else geotags.stored_nodata(geo, 16)
        out.update(overviews=args.out_overviews, resampling=args.out_resampling or "average", nodata=value)
    if args.out_georef is not None:
        out["geo"] = raster_io.read_geo_tags(args.out_georef) or None
    elif geo:
        out["geo"] = geo
    if V is not None:
        out["geo"] = with_nodata_tag(out.get("geo"), V, path)
    return out


def write_merged(path, image, out, geo=None):
    """a host array (merged tiles, gathered ranks) to its raster: uploaded once where --out-compress is given"""
    if out is None:
        write_plain(path, image, geo)
    else:
        raster_io.write_raster_device(path, ops.to_device_u16(image, DEVICE) if image.dtype == np.uint16 else
                                      torch.from_numpy(np.ascontiguousarray(image)).to(DEVICE), **out)


def log_comparison(org_img, rec_img, layer, args):
    """The records of `-org`: `MSE:` and `PSNR:` (peak fixed at 10000, ref decode.py:218), `Max error:` for a file with a
    residual layer (a file without one logs what it always logged), and with `--metrics` the lines of
    lbdrn_hip.quality.compare on the same two arrays behind them."""
    mse_value = np.mean((org_img.astype(np.float32) - rec_img.astype(np.float32)) ** 2)
    logger.log.info(f"MSE: {mse_value}")
    psnr = 10 * np.log10(10000 ** 2 / mse_value)
    logger.log.info(f"PSNR: {psnr}")
    if layer is not None:
        logger.log.info(f"Max error: {int(np.abs(org_img.astype(np.int64) - rec_img.astype(np.int64)).max())}")
    if args.metrics:
        from lbdrn_hip import quality
        q = quality.compare(org_img, rec_img, peak=args.metrics_peak if args.metrics_peak is not None else quality.DEFAULT_PEAK)
        for line in q.to_records():
            logger.log.info(line)
        if args.metrics_json is not None:
            with open(args.metrics_json, "w") as f:
                f.write(q.to_json())


def decode_window_main(args, rank, world):
    """`--window`: one part of the scene, bit-identical to that crop of the whole reconstruction.  Its records go to
    decode_window.txt: decode.txt, the marker of a finished whole decode, is neither read nor written."""
    dirname, basename = os.path.split(args.bin_path)
    dirname = dirname or "."
    if rank == 0:
        logger.create_logger(dirname, "decode_window.txt")
    else:
        logger.create_logger(dirname, "", log_file_only=True)
    logger.log.info(f"Binstream: {args.bin_path}")
    start_time = time.time()
    with open(args.bin_path, "rb") as fin:
        bitstream = fin.read()
    width, height = read_image_header(bitstream)[2:4]
    x0, y0, w, h = codec.check_window(args.window, width, height)
    logger.log.info(f"Window: x0={x0} y0={y0} w={w} h={h} of {width} x {height}")
    # the touched tiles are dealt over the ranks like all tiles of a whole decode
    layer = None if args.no_enhancement else container.unpack_residual_trailer(bitstream)      # (here for tau and the records only)
    if layer is not None:
        logger.log.info(f"Residual layer: max error {layer[0]}")
    # decode_window_pieces applies a layer by default; only --no-enhancement has anything to say to it
    more = {"enhance": False} if args.no_enhancement else {}
    masks = stored_mask(args, bitstream)
    V = masks[0] if masks is not None else None
    if V is not None:
        logger.log.info(f"Nodata: V={V}")
    if args.no_mask:
        more["mask"] = False
    _, parts = codec.decode_window_pieces(bitstream, args.window, device=DEVICE, take=lambda k, piece: k % world == rank, **more)
    recon_path = args.out_path or f"{dirname}/{basename[:-4]}_recon_x{x0}_y{y0}_w{w}_h{h}.tif"
    geo = stored_tags(args, bitstream, recon_path, (x0, y0, w, h))
    out = out_options(args, geo, V, recon_path)
    plain_geo = with_nodata_tag(geo, V, recon_path)
    on_device = out is not None and world == 1      # the pieces stay in HBM, are put together there and written from there
    if on_device:
        image = None
        for pc, rec in parts:
            if image is None:
                image = torch.zeros((rec.shape[0], h, w), dtype=rec.dtype, device=rec.device)
            image[:, pc.oy:pc.oy + rec.shape[1], pc.ox:pc.ox + rec.shape[2]] = rec
        raster_io.write_raster_device(recon_path, image, **out)
        gathered = []
        if args.org_path is not None:
            image = ops.from_device_u16(image)
    else:
        parts = [(pc.ox, pc.oy, ops.from_device_u16(rec)) for pc, rec in parts]
        gathered = shard.gather_to_root(parts) if world > 1 else [parts]
    if rank == 0:
        if not on_device:
            image = None
            for ox, oy, rec in (rec for part in gathered for rec in part):
                if image is None:
                    image = np.zeros((rec.shape[0], h, w), rec.dtype)
                image[:, oy:oy + rec.shape[1], ox:ox + rec.shape[2]] = rec
            write_merged(recon_path, image, out, plain_geo)
        logger.log.info(f"Recon: {recon_path}")
        if geo:
            logger.log.info(f"Tags: {len(geo)} tags restored")
        logger.log.info(f"Time elapsed: {time.time() - start_time}")
        if args.org_path is not None:
            org_img = raster_io.read_raster(args.org_path, window=(x0, y0, w, h))      # the window of the original alone
            org_img = org_img.reshape((-1,) + org_img.shape[-2:])
            log_comparison(org_img, image, layer, args)    # (no bpsp: a property of the whole file)
    if world > 1:
        shard.finish()
    return 0


def main(argv=None, shard_tiles=None):
    global K, D, bc, nl, DEVICE, ACTIVATION
    p = argparse.ArgumentParser(description="LBDRN-RSIC")
    p.add_argument("--seed", type=int, default=19920517)
    p.add_argument("-i", "--bin_path", type=str, help="binstream path")
    p.add_argument("-org", "--org_path", type=str, default=None, help="org path")
    p.add_argument("--window", type=int, nargs=4, default=None, metavar=("X0", "Y0", "W", "H"),
                   help="reconstruct this part of the scene only (scene pixels)")
    p.add_argument("--org-window", dest="org_window", type=int, nargs=4, default=None, metavar=("X0", "Y0", "W", "H"),
                   help="with -org: the file was encoded from this part of the original (encode.py --window)")
    p.add_argument("-o", "--out_path", type=str, default=None,
                   help="with --window: where the raster goes (default <name>_recon_x{X0}_y{Y0}_w{W}_h{H}.tif)")
    p.add_argument("--no-enhancement", dest="no_enhancement", action="store_true",
                   help="ignore the residual layer of a file that has one: the base reconstruction")
    p.add_argument("--no-mask", dest="no_mask", action="store_true",
                   help="ignore the nodata mask of a file that has one (encode.py --nodata): the reconstruction without the mask step")
    p.add_argument("--out-compress", dest="out_compress", choices=["deflate"], default=None,
                   help="write the reconstruction as a tiled, Deflate-compressed TIFF (predictor 2), compressed on the GPU")
    p.add_argument("--out-tile", dest="out_tile", type=int, default=None, metavar="N",
                   help="with --out-compress: N x N tiles (a multiple of 16; default 256)")
    p.add_argument("--out-overviews", dest="out_overviews", type=str, default=None, metavar="auto|N",
                   help="with --out-compress: add overview levels, reduced on the GPU (auto: until a level fits one tile)")
    p.add_argument("--out-resampling", dest="out_resampling", choices=["average", "nearest"], default=None,
                   help="with --out-overviews: how a level is reduced from the one before it (default average)")
    p.add_argument("--out-nodata", dest="out_nodata", type=int, default=None, metavar="V",
                   help="with --out-overviews: samples of this value do not enter an average")
    p.add_argument("--out-georef", dest="out_georef", type=str, default=None, metavar="FILE",
                   help="with --out-compress: copy FILE's georeferencing tags onto the output (the original scene, or any raster "
                        "on the same grid)")
    p.add_argument("--no-tags", dest="no_tags", action="store_true",
                   help="ignore the georeferencing tags of a file that carries them (encode.py --keep-tags): the raster a file "
                        "without them decodes to")
    p.add_argument("--metrics", action="store_true",
                   help="with -org: per-band error statistics, SSIM and the spectral angle, compared on the GPU (lbdrn_hip.quality)")
    p.add_argument("--metrics-peak", dest="metrics_peak", type=float, default=None, metavar="P",
                   help="with --metrics: the peak of its PSNR and SSIM (default 10000)")
    p.add_argument("--metrics-json", dest="metrics_json", type=str, default=None, metavar="FILE",
                   help="with --metrics: write every figure, histograms included, to FILE")
    args = p.parse_args(argv)
    if args.metrics and args.org_path is None:
        p.error("--metrics compares with the original: it goes with -org")
    if (args.metrics_peak is not None or args.metrics_json is not None) and not args.metrics:
        p.error("--metrics-peak and --metrics-json go with --metrics")
    if args.metrics_peak is not None and not (args.metrics_peak > 0 and np.isfinite(args.metrics_peak)):
        p.error(f"--metrics-peak {args.metrics_peak}: a positive finite number")
    if args.org_window is not None and (args.org_path is None or args.window is not None):
        p.error("--org-window goes with -org and a whole decode")
    if args.out_tile is not None and args.out_compress is None:
        p.error("--out-tile goes with --out-compress")
    if args.out_tile is not None and (args.out_tile < 16 or args.out_tile % 16):
        p.error(f"--out-tile {args.out_tile}: a tile side is a positive multiple of 16")
    for flag, value in (("--out-overviews", args.out_overviews), ("--out-resampling", args.out_resampling),
                        ("--out-nodata", args.out_nodata), ("--out-georef", args.out_georef)):
        if value is not None and args.out_compress is None:
            p.error(f"{flag} goes with --out-compress")
    if (args.out_resampling is not None or args.out_nodata is not None) and args.out_overviews is None:
        p.error("--out-resampling and --out-nodata go with --out-overviews")
    if args.out_overviews is not None:
        from lbdrn_hip import pyramid
        try:
            args.out_overviews = pyramid.parse_overviews(args.out_overviews)
        except ValueError:
            p.error(f"--out-overviews {args.out_overviews}: auto or a count of levels")
    if args.out_nodata is not None and not 0 <= args.out_nodata <= 65535:
        p.error(f"--out-nodata {args.out_nodata}: a sample value")
    if args.out_georef is not None and not os.path.exists(args.out_georef):
        p.error(f"--out-georef {args.out_georef}: no such file")
    if args.out_path is not None and args.window is None:
        p.error("-o names the raster of a --window decode")
    rank, world = 0, 1
    if shard_tiles is None:
        shard_tiles = shard.env_world()[1] > 1
    if shard_tiles:
        rank, world, local = shard.init_host_group()
        DEVICE = shard.bind_device(local)
    torch.manual_seed(args.seed)
    np.random.seed(args.seed)
    random.seed(args.seed)
    if args.window is not None:
        return decode_window_main(args, rank, world)
    dirname, basename = os.path.split(args.bin_path)
    dirname = dirname or "."
    filename = os.path.splitext(basename)[0]
    done = False
    if os.path.exists(f"{dirname}/decode.txt"):
        with open(f"{dirname}/decode.txt") as f:
            done = "bpsp" in f.read()
    if world > 1:
        done = all(shard.all_to_all_objects(done))
    if done:
        if rank == 0:
            print("Bitstream already decoded!")
        if world > 1:
            shard.finish()
        return 0
    if rank == 0:
        logger.create_logger(dirname, "decode.txt")
    else:
        logger.create_logger(dirname, "", log_file_only=True)
    logger.log.info(f"Binstream: {args.bin_path}")
    start_time = time.time()
    with open(args.bin_path, "rb") as fin:
        bitstream = fin.read()
    n_hdr, split_ratio, width, height, K, bc, nl, D, nn_list, base_list = read_image_header(bitstream)
    ACTIVATION = container.header_activation(bitstream)
    if ACTIVATION is not None and ACTIVATION != FeatCfg.from_constants().activation:
        logger.log.info(f"hidden activation {ACTIVATION} (from the header; constants.HIDDEN_ACTIVATION says otherwise)")
    layer = None if args.no_enhancement else container.unpack_residual_trailer(bitstream)
    if layer is not None:
        logger.log.info(f"Residual layer: max error {layer[0]}")
    bodies = layer[1] if layer is not None else [None] * (split_ratio * split_ratio)
    masks = stored_mask(args, bitstream)
    V = masks[0] if masks is not None else None
    if V is not None:
        logger.log.info(f"Nodata: V={V}")
    masks = [(V,) + entry for entry in masks[1]] if masks is not None else [None] * (split_ratio * split_ratio)
    recon_path = f"{dirname}/{basename[:-4]}_recon.tif"
    geo = stored_tags(args, bitstream, recon_path)
    out = out_options(args, geo, V, recon_path) if rank == 0 else None      # (rank 0 writes)
    plain_geo = with_nodata_tag(geo, V, recon_path)
    bitstream = bitstream[n_hdr:]
    if split_ratio > 1:
        decoded, offset = [], 0
        for t, (i, j, x0, y0, w, h) in enumerate(tile_windows(width, height, split_ratio)):
            if t % world == rank:
                test(bitstream[offset:], dirname, f"tile_{i}_{j}", nn_list[t], base_list[t], write=False, layer=bodies[t], mask=masks[t])
                decoded.append((t, test.last_image))
            offset += nn_list[t] + base_list[t]
        gathered = shard.gather_to_root(decoded) if world > 1 else [decoded]
        if rank == 0:
            tiles = dict(rec for part in gathered for rec in part)
            merged = None
            for t, (i, j, x0, y0, w, h) in enumerate(tile_windows(width, height, split_ratio)):
                if merged is None:
                    merged = np.zeros((tiles[t].shape[0], height, width), tiles[t].dtype)
                merged[:, y0:y0 + h, x0:x0 + w] = tiles[t]
            write_merged(recon_path, merged, out, plain_geo)
    elif rank == 0:
        test(bitstream, dirname, filename, nn_list[0], base_list[0], layer=bodies[0], out=out, geo=plain_geo, mask=masks[0])
    if rank == 0:
        if geo:
            logger.log.info(f"Tags: {len(geo)} tags restored")
        logger.log.info(f"Time elapsed: {time.time() - start_time}")
        if args.org_path is not None:
            org_img = (raster_io.read_raster(args.org_path) if args.org_window is None else
                       raster_io.read_raster(args.org_path, window=args.org_window))
            rec_img = raster_io.read_raster(recon_path)
            nbytes = os.path.getsize(args.bin_path)
            log_comparison(org_img, rec_img, layer, args)
            logger.log.info(f"Total size: {nbytes} bytes, bpsp={nbytes * 8 / np.prod(org_img.shape)}")
            os.remove(recon_path)                             # ref decode.py:223-224
    if world > 1:
        shard.finish()
    return 0


if __name__ == "__main__":
    sys.exit(main())
