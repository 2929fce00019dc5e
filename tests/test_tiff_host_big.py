"""The host build of csrc/tiff.inc (tests/tiff_host_shim.cpp, as tests/test_tiff_host.py compiles it) on segments of a scene's
size: every row of tests/tiff_big_cases.py -- zlib's level 1 / 6 / 9 / Z_FIXED streams of 128 KiB to 768 KiB segments,
hand-assembled Deflate blocks whose matches lie at the edge of the 32 KiB history ring, reach into stored blocks and use
codes of 11 to 15 bits, LZW and PackBits segments at their caps -- must end in status 0 and the exact bytes; the damaged
large segments must end in their status; the Adler-32 on non-zero data whose weights wrap.  No GPU: one lane of one.  The
device runs the same table in tests/test_gpu_tiff_big.py."""
import os
import sys
import zlib

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tiff_big_cases as B  # noqa: E402
import tiff_reference as R  # noqa: E402
from test_tiff_host import load_shim, shim_decode  # noqa: E402


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return load_shim(tmp_path_factory)


def test_the_table_holds_segments_at_the_caps_and_beyond_the_ring(shim):
    rows = B.rows()
    assert shim.tiff_shim_cap(R.COMP_DEFLATE) == B.CAP_DEFLATE and shim.tiff_shim_cap(R.COMP_LZW) == B.CAP_LZW
    by = {r[0]: r for r in rows}
    assert sum(len(r[3]) == B.CAP_DEFLATE for r in rows if r[1] == R.COMP_DEFLATE) == 4
    assert sum(len(r[3]) == B.CAP_LZW for r in rows if r[1] == R.COMP_LZW) == 3
    assert len(by["packbits-every-run"][3]) == 1 << 20
    for name, codec, stream, expected in rows:
        assert len(expected) > B.RING, name      # every segment is longer than the history ring
    # zlib's own streams use what the hand-made rows are built around: dynamic blocks with codes longer than the fast tables
    lit, dist = B.dynamic_code_lengths(by["zlib-tile256-9"][2])
    assert max(lit) > 10 and max(dist) >= 9, (max(lit), max(dist))


def test_host_build_decodes_every_row(shim):
    for name, codec, stream, expected in B.rows():
        st, got = shim_decode(shim, codec, stream, len(expected))
        assert st == 0, (name, st)
        assert got == expected, name


def test_host_build_flags_every_damaged_large_segment(shim):
    rows = B.damage_rows()
    assert len(rows) == 7
    for name, codec, bad, want, sound, expected in rows:
        assert len(expected) > B.RING
        assert shim_decode(shim, codec, sound, len(expected)) == (0, expected), name
        st, got = shim_decode(shim, codec, bad, len(expected))
        assert st != 0 and (want is None or st == want), (name, st)


def test_adler32_where_the_weights_wrap(shim):
    for data in B.ADLER_DATA():
        assert len(data) > 65521 and 0 not in data[:1000]
        assert shim.tiff_shim_adler32(data, len(data)) == zlib.adler32(data)
    assert any(len(d) > 2 * 65521 for d in B.ADLER_DATA())
