"""encode.py --max-error under a tile-sharded launch, on CPU (gloo, world_size 2): the residual bodies travel to rank 0 with
the other payloads and the file -- trailer included -- is byte-identical to the serial run's.  The GPU work (the fits, the
payload report and the layer's coder) is replaced by stand-ins whose output depends on the tile and on its weight payload,
like tests/test_cli_sharding_cpu.py does for the fits: what is under test is the plumbing around them."""
import hashlib
import os
import sys

import numpy as np
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "lbdrn-msic_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from test_cli_sharding_cpu import _records, _stub_report, _stub_train_tiles  # noqa: E402

ARGS = ["-sr", "3", "-K", "4", "-e", "2", "-bs", "64", "--max-error", "3"]
SUB = "scene_r3_K4_bc64_nl2_D2_prec16_lr0.001_bs64_e2"


def _stub_layer(args, res, tile, nn_payload):
    """Stands where encode.residual_layer stands (the closed loop on the GPU): a body that depends on the tile's pixels,
    on the weight payload it was coded against and on T, of a length that differs from tile to tile."""
    import logger
    h = hashlib.sha256(tile.tobytes() + bytes(nn_payload) + bytes([args.max_error])).digest()
    body = b"LBR1" + h * (1 + tile.shape[2] % 3) + tile.tobytes()[: tile.shape[1]]
    logger.log.info(f"Max error: {args.max_error}")
    logger.log.info(f"Residual layer: {len(body)} bytes: bpsp=0.125")
    return body


def _encode_worker(rank, world, port, src, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    import encode
    encode.train_tiles, encode.report_and_pack, encode.residual_layer = _stub_train_tiles, _stub_report, _stub_layer
    assert encode.main(["-i", src, "-o", out_dir] + ARGS) == 0


def test_tile_sharded_encode_with_a_layer_equals_serial(tmp_path, monkeypatch):
    import encode
    from lbdrn_hip import container
    src = str(tmp_path / "scene.npy")
    img = np.random.default_rng(4).integers(0, 9000, (2, 31, 40)).astype(np.uint16)
    np.save(src, img)
    monkeypatch.setattr(encode, "train_tiles", _stub_train_tiles)
    monkeypatch.setattr(encode, "report_and_pack", _stub_report)
    monkeypatch.setattr(encode, "residual_layer", _stub_layer)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert encode.main(["-i", src, "-o", str(tmp_path / "serial")] + ARGS) == 0
    assert encode.main(["-i", src, "-o", str(tmp_path / "plain")] + ARGS[:-2]) == 0
    mp.spawn(_encode_worker, args=(2, 29300 + os.getpid() % 250, src, str(tmp_path / "sharded")), nprocs=2, join=True)
    serial, sharded, plain = ((tmp_path / d / SUB / "scene.bin").read_bytes() for d in ("serial", "sharded", "plain"))
    assert serial == sharded
    # the trailer: T and the nine bodies in tile order, behind a file that is otherwise the one written without the flag
    off = container.residual_trailer_offset(serial)
    assert serial[:off] == plain and len(plain) == container.residual_trailer_offset(plain)
    assert container.unpack_residual_trailer(plain) is None
    tau, bodies = container.unpack_residual_trailer(sharded)
    assert tau == 3 and len(bodies) == 9 and len(set(bodies)) == 9 and len(set(map(len, bodies))) > 1
    from LBDRNdataset import tile_windows
    n_hdr, _, _, _, _, _, _, _, nn_list, base_list = container.unpack_header(sharded)
    at = n_hdr
    for (_, _, x0, y0, w, h), body, nn_bytes, base_bytes in zip(tile_windows(40, 31, 3), bodies, nn_list, base_list):
        tile = np.ascontiguousarray(img[:, y0:y0 + h, x0:x0 + w])
        assert body[4:36] == hashlib.sha256(tile.tobytes() + sharded[at:at + nn_bytes] + b"\x03").digest()
        at += nn_bytes + base_bytes
    # the records: the same, in tile order, each tile's layer behind its own payloads
    ra, rb = _records(tmp_path / "serial" / SUB / "encode.txt"), _records(tmp_path / "sharded" / SUB / "encode.txt")
    strip = lambda recs: [r.replace(str(tmp_path / "serial"), "X").replace(str(tmp_path / "sharded"), "X")
                          for r in recs if not r.startswith("Time elapsed")]
    assert strip(ra) == strip(rb)
    kinds = [r.split(":")[0] for r in rb if r.startswith(("nn: ", "MSB: ", "Max error: ", "Residual layer: "))]
    assert kinds == ["nn", "MSB", "Max error", "Residual layer"] * 9
