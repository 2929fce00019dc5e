#!/bin/bash
# (host) The GPU JPEG 2000 decoder's host-compilable text (csrc/jp2k_t1d.inc, csrc/jp2k_t2d.inc through
# tests/jp2k_dec_host_shim.cpp) rebuilt with AddressSanitizer + UndefinedBehaviorSanitizer (first finding aborts) and put
# under the CPU tests that drive it: the block fuzz at every pass count and every prefix, the packet headers, whole files,
# 400 truncations and 1000 single-byte corruptions.  The shim is compiled into the tests' temporary directory, so there is
# no regular build to restore.  scripts/sanitize_cpu.sh is the same for the oracle and the OpenJPEG shim.
#     bash scripts/sanitize_jp2k_dec.sh
set -u
cd "$(dirname "$0")/.."
ASAN=$(g++ -print-file-name=libasan.so)
LBDRN_JP2K_DEC_SHIM_SANITIZE=1 LD_PRELOAD="$ASAN${LD_PRELOAD:+:$LD_PRELOAD}" ASAN_OPTIONS=detect_leaks=0 \
  python -m pytest tests/test_jp2k_dec_host.py -x -q -m "not gpu" -k "block_decoder or packet_header or block_table or tile_parts or truncated" || exit 1
# the same for files with a precinct partition and the component transform (Pillow's, tests/golden/jp2k_precincts.npz)
LBDRN_JP2K_DEC_SHIM_SANITIZE=1 LD_PRELOAD="$ASAN${LD_PRELOAD:+:$LD_PRELOAD}" ASAN_OPTIONS=detect_leaks=0 \
  python -m pytest tests/test_jp2k_dec_precincts_host.py -x -q -m "not gpu" -k "not pillow_writes"
