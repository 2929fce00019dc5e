"""Host logic of the K points of an image fitted side by side (sweep.py --k-in-flight, encode.main_k_points, codec.fit_many
with a K list), on the CPU: the device work is replaced by stand-ins whose output depends on the tile, on K and on the random
draws made for the tile (in the manner of tests/test_resid_sharding_cpu.py) -- what is under test is everything around it."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "lbdrn-msic_amd")
for p in (PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_cli_sharding_cpu import _records, _stub_report  # noqa: E402


def _payloads(img, K, dr):
    h = hashlib.sha256(dr.params.numpy().tobytes() + repr(dr.train_seeds).encode() + bytes([K])).digest()
    return h + hashlib.sha256(img.tobytes()).digest(), (img >> K).tobytes()[: 50 + img.shape[2]]


def _stub_train_tiles(args, tiles, draws):
    """Stands where encode.train_tiles stands (main's fits)."""
    return [_payloads(img, args.K, dr) for (_, img), dr in zip(tiles, draws)]


def _stub_train_tiles_at(args, arrays, Ks, draws):
    """Stands where encode.train_tiles_at stands (main_k_points' fits).  K = 5 ends with an exception where the test asks."""
    return [RuntimeError("no epoch improved") if K == _stub_train_tiles_at.fail else _payloads(img, K, dr)
            for img, K, dr in zip(arrays, Ks, draws)]


_stub_train_tiles_at.fail = None


def test_buckets_by_image_at_world_sizes_1_2_3():
    import sweep
    from lbdrn_hip import shard
    a = sweep.parse(["--images", "a.tif", "b.tif", "--k", "1", "6", "--k-in-flight", "4"])
    todo = sweep.points(a)
    at = lambda idxs: [todo[i] for i in idxs]
    # one rank: every image's six points, four and two
    got = sweep.buckets(todo, shard.assign(len(todo), 0, 1), 4)
    assert [at(b) for b in got] == [[("a.tif", 1), ("a.tif", 2), ("a.tif", 3), ("a.tif", 4)], [("a.tif", 5), ("a.tif", 6)],
                                    [("b.tif", 1), ("b.tif", 2), ("b.tif", 3), ("b.tif", 4)], [("b.tif", 5), ("b.tif", 6)]]
    # two ranks: dealing stays per point (odd / even K), a rank buckets what it was dealt
    got = [sweep.buckets(todo, shard.assign(len(todo), r, 2), 4) for r in range(2)]
    assert [at(b) for b in got[0]] == [[("a.tif", 1), ("a.tif", 3), ("a.tif", 5)], [("b.tif", 1), ("b.tif", 3), ("b.tif", 5)]]
    assert [at(b) for b in got[1]] == [[("a.tif", 2), ("a.tif", 4), ("a.tif", 6)], [("b.tif", 2), ("b.tif", 4), ("b.tif", 6)]]
    # three ranks, two in flight
    got = [sweep.buckets(todo, shard.assign(len(todo), r, 3), 2) for r in range(3)]
    assert [at(b) for b in got[0]] == [[("a.tif", 1), ("a.tif", 4)], [("b.tif", 1), ("b.tif", 4)]]
    assert [at(b) for b in got[2]] == [[("a.tif", 3), ("a.tif", 6)], [("b.tif", 3), ("b.tif", 6)]]
    for world, n in ((1, 4), (2, 4), (3, 2), (3, 1), (5, 6)):
        parts = [sweep.buckets(todo, shard.assign(len(todo), r, world), n) for r in range(world)]
        flat = [i for part in parts for b in part for i in b]
        assert sorted(flat) == list(range(len(todo)))                              # every point once
        for part in parts:
            assert all(1 <= len(b) <= n and len({todo[i][0] for i in b}) == 1 and b == sorted(b) for b in part)
            assert [b[0] for b in part] == sorted(b[0] for b in part)              # run.sh's order


def test_option_parse_and_the_positional_form():
    import sweep
    assert sweep.parse(["--images", "a.tif"]).k_in_flight == 1
    assert sweep.parse(["--images", "a.tif", "--k-in-flight", "6"]).k_in_flight == 6
    a = sweep.parse(["3", "2", "256", "2", "0.001", "8192", "10", "1", "outputs-x", "--k-in-flight", "6"])      # run.sh's form
    assert (a.D, a.base_channel, a.epochs, a.split_ratio, a.output_dir, a.k_in_flight) == (2, 256, 10, 1, "outputs-x", 6)
    with pytest.raises(SystemExit):
        sweep.parse(["--images", "a.tif", "--k-in-flight", "0"])


def test_run_sh_passes_the_option_through(tmp_path):
    """run.sh with K_IN_FLIGHT=6 hands `--k-in-flight 6` to sweep.py behind its nine positional arguments; without the
    variable the command line is today's.  (`python` is a stand-in that prints its arguments.)"""
    fake = tmp_path / "python"
    fake.write_text('#!/bin/bash\nprintf "%s\\n" "$@"\n')
    fake.chmod(0o755)
    positional = ["0", "2", "64", "2", "0.001", "8192", "10", "1", "outputs"]
    env = {k: v for k, v in os.environ.items() if k not in ("NGPU", "K_IN_FLIGHT", "PER_GPU")}
    env.update(PATH=f"{tmp_path}:{env['PATH']}", PER_GPU="1")
    run = lambda e: subprocess.run(["bash", os.path.join(PKG, "run.sh")] + positional, env=e, capture_output=True, text=True,
                                   check=True).stdout.split("\n")[:-1]
    plain = run(env)
    assert plain == [os.path.join(PKG, "sweep.py")] + positional
    got = run(dict(env, K_IN_FLIGHT="6"))
    assert got == plain + ["--k-in-flight", "6"]
    import sweep
    assert sweep.parse(got[1:]).k_in_flight == 6


class _Sweep:
    """sweep.main with stand-ins for the encoder and the decoder: what it called, in order."""

    def __init__(self, monkeypatch, fail=()):
        import sweep
        encode, decode = sweep.encode, sweep.decode      # (the modules sweep.py itself calls into)
        self.calls = []

        def enc_main(argv, shard_tiles=None):
            K = int(argv[argv.index("-K") + 1])
            self.calls.append(("encode.main", argv[argv.index("-i") + 1], K))
            if K in fail:
                raise RuntimeError(f"K={K} fails")
            return 0

        def enc_many(argv, Ks):
            assert "-K" not in argv
            self.calls.append(("encode.main_k_points", argv[argv.index("-i") + 1], tuple(Ks)))
            return {K: (RuntimeError(f"K={K} fails") if K in fail else None) for K in Ks}

        def dec_main(argv, shard_tiles=None):
            self.calls.append(("decode.main", os.path.basename(os.path.dirname(argv[argv.index("-i") + 1]))))
            return 0
        monkeypatch.setattr(encode, "main", enc_main)
        monkeypatch.setattr(encode, "main_k_points", enc_many)
        monkeypatch.setattr(decode, "main", dec_main)
        for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
            monkeypatch.delenv(k, raising=False)
        self.main = sweep.main


def test_records_their_order_and_the_default_path(monkeypatch, capsys):
    args = ["--images", "x/a.tif", "y/b.tif", "--k", "2", "5", "-o", "out"]
    folder = lambda stem, K: f"{stem}_r1_K{K}_bc64_nl2_D2_prec16_lr0.001_bs8192_e10"
    # N = 1 (the default, and spelled out): today's loop -- encode.main then decode.main per point, never the new function
    for extra in ([], ["--k-in-flight", "1"]):
        s = _Sweep(monkeypatch)
        assert s.main(args + extra) == 0
        want = []
        for image, stem in (("x/a.tif", "a"), ("y/b.tif", "b")):
            for K in (2, 3, 4, 5):
                want += [("encode.main", image, K), ("decode.main", folder(stem, K))]
        assert s.calls == want
        plain = [line for line in capsys.readouterr().out.splitlines() if " K=" in line and not line.startswith("[rank")]
    assert [line.split(":")[0] for line in plain] == [f"{n} K={K}" for n in ("a.tif", "b.tif") for K in (2, 3, 4, 5)]
    # N = 3: three and one of every image through the new function, each bucket decoded point after point
    s = _Sweep(monkeypatch)
    assert s.main(args + ["--k-in-flight", "3"]) == 0
    want = []
    for image, stem in (("x/a.tif", "a"), ("y/b.tif", "b")):
        for Ks in ((2, 3, 4), (5,)):
            want += [("encode.main_k_points", image, Ks)] + [("decode.main", folder(stem, K)) for K in Ks]
    assert s.calls == want
    out = capsys.readouterr().out.splitlines()
    grouped = [line for line in out if " K=" in line and not line.startswith("[rank")]
    strip = lambda lines: [line.rsplit(" in ", 1)[0] for line in lines]
    assert strip(grouped) == strip(plain) and out[-1] == "All files processed."           # the same records in the same order
    # a point that fails is reported, the others finish, the exit status says so -- as in the default loop
    for extra in ([], ["--k-in-flight", "4"]):
        s = _Sweep(monkeypatch, fail=(3,))
        assert s.main(args + extra) == 1
        lines = [line for line in capsys.readouterr().out.splitlines() if " K=" in line and not line.startswith("[rank")]
        assert [("FAILED (RuntimeError: K=3 fails)" in line) for line in lines] == [False, True, False, False] * 2
        assert [c[1] for c in s.calls if c[0] == "decode.main"] == [folder(n, K) for n in "ab" for K in (2, 4, 5)]


def test_main_k_points_writes_what_main_writes_point_after_point(tmp_path, monkeypatch):
    """Stand-in fits whose payloads depend on the tile, on K and on the tile's draws: drawing once per tile for all K gives
    what every re-seeded main() draws; three tiles a side; with and without a (stand-in) residual layer."""
    import encode
    from test_resid_sharding_cpu import _stub_layer
    src = str(tmp_path / "scene.npy")
    np.save(src, np.random.default_rng(4).integers(0, 9000, (2, 31, 40)).astype(np.uint16))
    monkeypatch.setattr(encode, "train_tiles", _stub_train_tiles)
    monkeypatch.setattr(encode, "train_tiles_at", _stub_train_tiles_at)
    monkeypatch.setattr(encode, "report_and_pack", _stub_report)
    monkeypatch.setattr(encode, "residual_layer", _stub_layer)
    monkeypatch.setattr(encode, "BASE_CODEC", "LBB2")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    Ks = (3, 4, 5, 6)
    for tag, extra in (("plain", []), ("layer", ["--max-error", "3"])):
        common = ["-sr", "3", "-e", "2", "-bs", "64"] + extra
        one, many = tmp_path / f"one-{tag}", tmp_path / f"many-{tag}"
        for K in Ks:
            assert encode.main(["-i", src, "-o", str(one), "-K", str(K)] + common, shard_tiles=False) == 0
        assert encode.main_k_points(["-i", src, "-o", str(many), "-K", "9"] + common, Ks) == {K: None for K in Ks}    # (-K: ignored)
        for K in Ks:
            sub = f"scene_r3_K{K}_bc64_nl2_D2_prec16_lr0.001_bs64_e2"
            assert (one / sub / "scene.bin").read_bytes() == (many / sub / "scene.bin").read_bytes(), (tag, K)
            ra, rb = _records(one / sub / "encode.txt"), _records(many / sub / "encode.txt")
            strip = lambda recs, root: [r.replace(str(root), "X") for r in recs if not r.startswith("Time elapsed")]
            assert strip(ra, one) == strip(rb, many) and rb[-1].startswith("Time elapsed: "), (tag, K)
    # a point whose fit fails is that point's exception; the others are written
    _stub_train_tiles_at.fail = 5
    try:
        out = encode.main_k_points(["-i", src, "-o", str(tmp_path / "fail"), "-sr", "3", "-e", "2", "-bs", "64"], Ks)
    finally:
        _stub_train_tiles_at.fail = None
    assert [type(out[K]) for K in Ks] == [type(None), type(None), RuntimeError, type(None)]
    for K in Ks:
        sub = f"scene_r3_K{K}_bc64_nl2_D2_prec16_lr0.001_bs64_e2"
        assert (tmp_path / "fail" / sub / "scene.bin").exists() == (K != 5)
        if K != 5:
            assert (tmp_path / "fail" / sub / "scene.bin").read_bytes() == (tmp_path / "one-plain" / sub / "scene.bin").read_bytes()


class _T:
    """what fit_many's job formation and the memory limiter look at of a device tensor"""

    def __init__(self, ptr, *shape):
        self.ptr, self.shape, self.device = ptr, shape, "cuda:0"

    def data_ptr(self):
        return self.ptr


def test_job_formation_with_a_k_list():
    from lbdrn_hip import codec
    a, b, c = _T(1, 4, 24, 26), _T(2, 4, 24, 25), _T(3, 4, 24, 26)
    # the K points of tile a, then of tile b (another shape), then of c (a's shape again): tile-major, as main_k_points orders them
    images = [a] * 4 + [b] * 3 + [c]
    Ks = [3, 4, 5, 6, 3, 4, 5, 3]
    draws = ["da"] * 4 + ["db"] * 3 + ["dc"]
    jobs = codec.form_jobs(images, draws, Ks, 2)
    assert [j[0] for j in jobs] == [[0, 1], [2, 3], [4, 5], [6], [7]]              # mixed K of one shape pair up; a shape change splits
    assert [j[3] for j in jobs] == [[3, 4], [5, 6], [3, 4], [5], [3]]
    assert all(j[1] == [images[i] for i in j[0]] and j[2] == [draws[i] for i in j[0]] for j in jobs)
    assert [j[0] for j in codec.form_jobs(images, draws, Ks, 4)] == [[0, 1, 2, 3], [4, 5, 6], [7]]
    assert [j[0] for j in codec.form_jobs(images, draws, Ks, 1)] == [[k] for k in range(8)]
    # one shape throughout, different images: K does not split
    assert [j[0] for j in codec.form_jobs([a, c, a, c], [None] * 4, [1, 6, 2, 5], 2)] == [[0, 1], [2, 3]]
    assert codec.k_per_fit(5, 3) == [5, 5, 5] and codec.k_per_fit((1, 2), 2) == [1, 2]
    with pytest.raises(ValueError):
        codec.k_per_fit([1, 2], 3)


def test_one_image_at_several_k_is_counted_once_against_the_memory(monkeypatch):
    import torch
    from lbdrn_hip import codec
    # the arithmetic: need 10 per fit of which 4 are the image
    fit = codec.in_flight_that_fit
    assert fit([1, 2, 3, 4], 10, 4, 40, 4) == 4 and fit([1, 2, 3, 4], 10, 4, 39, 4) == 3      # distinct images: budget // need
    assert fit([1, 1, 1, 1], 10, 4, 28, 4) == 4 and fit([1, 1, 1, 1], 10, 4, 27, 4) == 3      # one image: 6 m + 4
    assert fit([1, 1, 2, 2], 10, 4, 28, 4) == 3 and fit([1, 1, 2, 2], 10, 4, 32, 4) == 4      # the run with most images decides
    assert fit([1, 1], 10, 4, 100, 4) == 4                                                     # (more wanted than fits there are: as before)
    assert fit([1, 1], 10, 4, 9, 4) == 0
    # through memory_limited_in_flight at the reference's scene sizes, a 288 GB part with 280 GiB free
    monkeypatch.delenv("LBDRN_DEVICE_SHARED", raising=False)
    monkeypatch.setattr(torch.cuda, "memory_reserved", lambda dev=None: 0)
    monkeypatch.setattr(torch.cuda, "memory_allocated", lambda dev=None: 0)
    args = (2, 64, 2, 8192, 10)
    Ks = [1, 2, 3, 4, 5, 6]
    big = codec.fit_bytes(8, 6000, 6000, Ks, *args)
    assert big == codec.fit_bytes(8, 6000, 6000, 5, *args) and codec.image_bytes(8, 6000, 6000) == 8 * 6000 * 6000 * 2
    scene = _T(7, 8, 6000, 6000)
    others = [_T(10 + k, 8, 6000, 6000) for k in range(6)]
    budget = 5 * (big - codec.image_bytes(8, 6000, 6000)) + codec.image_bytes(8, 6000, 6000)     # five fits of ONE scene exactly
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (int(budget / 0.85) + 2, 288 << 30))
    assert codec.memory_limited_in_flight([scene] * 6, 6, Ks, *args) == 5
    assert codec.memory_limited_in_flight(others, 6, Ks, *args) == 4                              # six scenes: 4 x 34 GiB
    assert codec.memory_limited_in_flight(others, 6, 5, *args) == 4                               # (an int K: the same)
    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda dev=None: (280 << 30, 288 << 30))
    assert codec.memory_limited_in_flight([scene] * 6, 6, Ks, *args) == 6
    assert codec.memory_limited_in_flight([_T(8, 4, 7550, 7550)] * 6, 6, Ks, *args) == 6
    assert codec.default_in_flight(8, 2048, 2048, Ks, 2, 64, 2) == 4
