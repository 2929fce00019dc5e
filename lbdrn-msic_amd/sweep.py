"""The K-sweep of the reference's run.sh (ref run.sh:29-42) as one multi-GPU job.

run.sh loops images x K = 1..6 serially on one device, starting two Python processes per point.  Every
(image, K) point is an independent encode + decode that re-seeds its RNG (ref encode.py:200-205), so here the
points are dealt round-robin to the ranks of a torchrun launch -- one process per GPU, no exchange between
points -- and each rank runs its points in-process (the HIP library and the CUDA context are loaded once).
Rank 0 gathers one small record per point at the end and, with --summary, writes the CSV of
results_summary.py.

    python -m torch.distributed.run --nproc-per-node 8 sweep.py -o outputs --images data/*.tif
    python sweep.py -o outputs --images a.tif b.tif --k 1 6            # single GPU

--k-in-flight N (default 1: the loop above, point after point): a rank fits up to N of the K points it was dealt of one
image side by side on its GPU (encode.main_k_points -- one raster, one set of draws, one launch per minibatch for a pair
of K's) and then decodes them one after another; files, records and the CSV are those of the default.

The positional form of run.sh is kept too:  sweep.py DEVICE_ID D BC NL LR BS EPOCH SR OUTPUT_DIR
(run.sh exports HIP_VISIBLE_DEVICES=DEVICE_ID unless NGPU is set; sweep.py itself takes its device from the launcher).
"""
import argparse
import os
import sys
import time
import traceback

import decode
import encode
import results_summary
from lbdrn_hip import shard

REFERENCE_IMAGES = (
    [f"data/GF-dataset/GF-2/{name}.tif" for name in results_summary.TRIPLESAT]
    + [f"data/GF-dataset/GF-6/GF6-{s}/GF6_{s}_Sample_{x}.tif" for s in ("WFI", "PMS") for x in "ABCD"]
)


def build_parser():
    p = argparse.ArgumentParser(description="LBDRN-MSIC K sweep (encode + decode per point)")
    p.add_argument("legacy", nargs="*", help="run.sh form: DEVICE_ID D BC NL LR BS EPOCH SR OUTPUT_DIR")
    p.add_argument("--images", nargs="*", default=None, help="input rasters (default: the reference's list)")
    p.add_argument("--k", nargs=2, type=int, default=(1, 6), metavar=("FIRST", "LAST"), help="inclusive K range")
    p.add_argument("-o", "--output_dir", default="outputs")
    p.add_argument("-sr", "--split_ratio", type=int, default=1)
    p.add_argument("-bc", "--base_channel", type=int, default=64)
    p.add_argument("-nl", "--num_layers", type=int, default=2)
    p.add_argument("-D", "--D", type=int, default=2)
    p.add_argument("-prec", "--precision", type=int, default=16)
    p.add_argument("-lr", "--lr", type=str, default="0.001", help="kept as text: it is part of the directory name")
    p.add_argument("-bs", "--batch_size", type=int, default=8192)
    p.add_argument("-e", "--epochs", type=int, default=10)
    p.add_argument("--window", type=int, nargs=4, default=None, metavar=("X0", "Y0", "W", "H"),
                   help="sweep this part of every image only (encode.py --window)")
    p.add_argument("--keep-tags", dest="keep_tags", action="store_true",
                   help="every .bin carries its image's georeferencing and nodata tags (encode.py --keep-tags)")
    p.add_argument("--nodata", dest="nodata", type=str, default=None, metavar="V|tag",
                   help="every .bin keeps samples of this value exact (encode.py --nodata; tag: each image's GDAL_NODATA)")
    p.add_argument("--nodata-fit", dest="nodata_fit", choices=("all", "valid"), default=None,
                   help="with --nodata: `valid` fits and ranks on the valid pixels only (encode.py --nodata-fit)")
    p.add_argument("--summary", action="store_true", help="rank 0 writes the results CSV at the end")
    p.add_argument("--k-in-flight", dest="k_in_flight", type=int, default=1, metavar="N",
                   help="fit up to N of the K points of an image side by side on the GPU (encode.main_k_points); "
                        "default 1: point after point.  Same files and records either way")
    return p


def parse(argv=None):
    a = build_parser().parse_args(argv)
    if a.legacy:
        if len(a.legacy) != 9:
            raise SystemExit("positional form takes exactly: DEVICE_ID D BC NL LR BS EPOCH SR OUTPUT_DIR")
        _, D, BC, NL, LR, BS, EPOCH, SR, OUT = a.legacy
        a.D, a.base_channel, a.num_layers, a.lr = int(D), int(BC), int(NL), LR
        a.batch_size, a.epochs, a.split_ratio, a.output_dir = int(BS), int(EPOCH), int(SR), OUT
    a.images = a.images if a.images else list(REFERENCE_IMAGES)
    if a.k_in_flight < 1:
        raise SystemExit(f"--k-in-flight {a.k_in_flight}: 1 (point after point) or more")
    if a.nodata_fit == "valid" and a.nodata is None:   # before any fit of the sweep starts, as encode.py refuses it
        raise SystemExit("--nodata-fit valid needs --nodata V|tag")
    if os.environ.get("LBDRN_WEIGHTS_CODEC") != "fpzip":
        from lbdrn_hip import container
        try:   # before any fit of the sweep starts
            container.check_weight_precision(a.precision)
        except ValueError as e:
            raise SystemExit(str(e))
    return a


def points(a):
    """The sweep in run.sh's order: images outermost, K inside."""
    return [(img, K) for img in a.images for K in range(a.k[0], a.k[1] + 1)]


def common_args(a):
    return (["-D", str(a.D), "-bc", str(a.base_channel), "-nl", str(a.num_layers),
            "-lr", a.lr, "-bs", str(a.batch_size), "-e", str(a.epochs), "-sr", str(a.split_ratio),
            "-prec", str(a.precision)] + window_args(a, "--window") + (["--keep-tags"] if getattr(a, "keep_tags", False) else [])
            + (["--nodata", str(a.nodata)] if getattr(a, "nodata", None) is not None else [])
            + (["--nodata-fit", a.nodata_fit] if getattr(a, "nodata_fit", None) is not None else []))


def window_args(a, flag):
    win = getattr(a, "window", None)
    return [] if win is None else [flag] + [str(v) for v in win]


def point_stem(a, image):
    """encode.scene_name: the image's stem, with --window the window behind it"""
    stem = os.path.splitext(os.path.basename(image))[0]
    win = getattr(a, "window", None)
    return stem if win is None else stem + "_x{}_y{}_w{}_h{}".format(*win)


def point_folder(a, image, K):
    # float(lr) -> the directory name encode.py derives from its parsed float (ref run.sh:38 spells it by hand)
    stem = point_stem(a, image)
    return (f"{a.output_dir}/{stem}_r{a.split_ratio}_K{K}_bc{a.base_channel}_nl{a.num_layers}_D{a.D}"
            f"_prec{a.precision}_lr{float(a.lr)}_bs{a.batch_size}_e{a.epochs}")


def decode_point(a, image, K):
    stem = point_stem(a, image)
    folder = point_folder(a, image, K)
    decode.main(["-i", f"{folder}/{stem}.bin", "-org", image] + window_args(a, "--org-window"), shard_tiles=False)
    return folder


def run_point(a, image, K):
    encode.main(["-i", image, "-o", a.output_dir, "-K", str(K)] + common_args(a), shard_tiles=False)
    return decode_point(a, image, K)


def buckets(todo, mine, k_in_flight):
    """The points a rank was dealt (`mine`: indices into `todo`, ascending = run.sh's order), bucketed by image: up to
    k_in_flight points of one image each, in that order -> [[index, ...], ...].  Dealing over the ranks stays per
    point; a rank that holds K = 1, 3, 5 of an image fits those three together."""
    by_image = {}
    for idx in mine:
        by_image.setdefault(todo[idx][0], []).append(idx)
    out = []
    for idxs in by_image.values():
        out += [idxs[k:k + k_in_flight] for k in range(0, len(idxs), k_in_flight)]
    return out


def run_bucket(a, rank, todo, idxs):
    """Encode the K points todo[idxs] of one image together (encode.main_k_points), then decode them one after another
    as run_point does -> one record per point, in idxs order.  A point's seconds: its share of the encode all of them
    did together, plus its own decode."""
    image = todo[idxs[0]][0]
    Ks = [todo[idx][1] for idx in idxs]
    t0 = time.time()
    for K in Ks:
        print(f"[rank {rank}] Processing file: {image}  K={K}", flush=True)
    try:
        outcome = encode.main_k_points(["-i", image, "-o", a.output_dir] + common_args(a), Ks)
    except Exception as e:
        outcome = {K: e for K in Ks}
    share = (time.time() - t0) / len(Ks)
    records = []
    for idx, K in zip(idxs, Ks):
        t1 = time.time()
        folder, e = None, outcome.get(K)
        if e is None:
            try:
                folder = decode_point(a, image, K)
            except Exception as e_:
                e = e_
        if e is not None:      # run.sh carries on after a failed point; so does the sweep
            traceback.print_exception(type(e), e, e.__traceback__)
        records.append((idx, image, K, folder, None if e is None else f"{type(e).__name__}: {e}", share + time.time() - t1))
    return records


def main(argv=None):
    a = parse(argv)
    rank, world, local = shard.init_host_group()
    encode.DEVICE = decode.DEVICE = shard.bind_device(local)
    todo = points(a)
    records = []
    mine = shard.assign(len(todo), rank, world)
    if a.k_in_flight > 1:
        for idxs in buckets(todo, mine, a.k_in_flight):
            records += run_bucket(a, rank, todo, idxs)
        records.sort()      # (run.sh's order, like the loop below)
        mine = []
    for idx in mine:
        image, K = todo[idx]
        t0 = time.time()
        print(f"[rank {rank}] Processing file: {image}  K={K}", flush=True)
        try:
            folder, err = run_point(a, image, K), None
        except Exception as e:   # run.sh carries on after a failed point; so does the sweep
            traceback.print_exc()
            folder, err = None, f"{type(e).__name__}: {e}"
        records.append((idx, image, K, folder, err, time.time() - t0))
    gathered = shard.gather_to_root(records)
    failed = 0
    if rank == 0:
        for idx, image, K, folder, err, secs in sorted(rec for part in gathered for rec in part):
            status = "ok" if err is None else f"FAILED ({err})"
            print(f"{os.path.basename(image)} K={K}: {status} in {secs:.1f}s")
            failed += err is not None
        print("All files processed.")
        if a.summary:
            stems = [point_stem(a, i) for i in a.images]
            results_summary.save_to_csv(
                ["-o", a.output_dir, "-sr", str(a.split_ratio), "-bc", str(a.base_channel), "-nl", str(a.num_layers),
                 "-D", str(a.D), "-prec", str(a.precision), "-lr", a.lr, "-bs", str(a.batch_size),
                 "-e", str(a.epochs), "--k", str(a.k[0]), str(a.k[1]), "--files"] + stems)
    if world > 1:
        failed = sum(shard.all_to_all_objects(failed))
        shard.finish()
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
