"""The CPU half of the lbdrn_randperm tests: a plain numpy restatement of torch.randperm on a seeded CPU generator
(MT19937 + the forward Fisher-Yates pass), a census of how many steps target each position, the constants of
csrc/randperm.hip read out of its text, and the (seed, n) pairs and sizes tests/test_gpu_randperm.py runs on the device.

Nothing here needs a GPU.  What is proven here is what the GPU tests rely on without looking again: that the restatement
equals torch, that every pair reaches the list branch of k_links / k_part_links it was chosen for, that every edge size
is still the edge it is named after (a change of a constant in the kernel source fails HERE instead of quietly moving
the edge out from under its test), and that sampler.epoch_plan / draw_pass_seeds consume the global generator exactly
as a DataLoader(shuffle=True) that is iterated once per training pass and once per evaluation pass."""
import functools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_SOURCE = os.path.join(ROOT, "lbdrn-msic_amd", "csrc", "randperm.hip")


# ---------------------------------------------------------------------------------------------------------------------
# the plain reference

def mt19937_outputs(seed, count):
    """The first `count` 32-bit outputs of mt19937ar seeded by init_genrand(seed & 0xffffffff) (what at::mt19937(seed)
    is): the state regenerated 624 words at a time in three slices (the recurrence reaches back 227 words), then
    tempered."""
    n, m = 624, 397
    blocks = (count + n - 1) // n
    x = np.zeros((blocks + 1) * n, np.uint32)
    v = seed & 0xFFFFFFFF
    x[0] = v
    for k in range(1, n):
        v = (1812433253 * (v ^ (v >> 30)) + k) & 0xFFFFFFFF
        x[k] = v
    one, upper, lower, magic = np.uint32(1), np.uint32(0x80000000), np.uint32(0x7FFFFFFF), np.uint32(0x9908B0DF)
    for base in range(0, blocks * n, n):
        for lo, hi in ((0, 227), (227, 454), (454, 624)):
            a, b, c = x[base + lo:base + hi], x[base + lo + 1:base + hi + 1], x[base + lo + m:base + hi + m]
            y = (a & upper) | (b & lower)
            x[base + n + lo:base + n + hi] = c ^ (y >> one) ^ np.where(b & one, magic, np.uint32(0))
    y = x[n:n + count].copy()
    y ^= y >> np.uint32(11)
    y ^= (y << np.uint32(7)) & np.uint32(0x9D2C5680)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    y ^= y >> np.uint32(18)
    return y


def targets(seed, n):
    """j_i = i + out_i % (n - i) for i < n - 1: the position step i of the Fisher-Yates pass swaps position i with."""
    steps = max(n - 1, 0)
    i = np.arange(steps, dtype=np.int64)
    return i + mt19937_outputs(seed, steps).astype(np.int64) % (n - i)


def fisher_yates(j, n):
    """The sequential pass itself: r = 0 .. n-1, then swap(r[i], r[j_i]) for i = 0 .. n-2, in order."""
    r = list(range(n))
    for i, t in enumerate(j.tolist()):
        r[i], r[t] = r[t], r[i]
    return np.asarray(r, np.int64)


def reference_randperm(seed, n):
    return fisher_yates(targets(seed, n), n)


@functools.lru_cache(maxsize=None)
def census(seed, n):
    """count[p] = the number of steps whose target is position p: the length of p's list in k_links / k_part_links."""
    c = np.bincount(targets(seed, n), minlength=n)
    c.setflags(write=False)
    return c


def torch_randperm(seed, n):
    g = torch.Generator()
    g.manual_seed(seed)
    return torch.randperm(n, generator=g)


# ---------------------------------------------------------------------------------------------------------------------
# the constants of csrc/randperm.hip, out of its text

def kernel_constants(text=None):
    """LINK_REG, LINK_LDS, PART_SHIFT, PART_MAX, PART_CHUNK as the source states them, PART_ENTER = the factor of
    "n > PART_ENTER * PART_SIZE" in perm_partitioned(), SCAN_TURN = the entries k_part_scan_rows scans per turn of its
    loop, CALL_MAX = the seeds one library call takes.  PART_SIZE and PART_MAX_N are derived the way the source derives
    them, and that derivation is matched as text too."""
    if text is None:
        with open(KERNEL_SOURCE) as f:
            text = f.read()
    k = {}
    for name in ("LINK_REG", "LINK_LDS", "PART_SHIFT", "PART_MAX", "PART_CHUNK"):
        found = re.findall(r"\b%s = (\d+)\b" % name, text)
        assert len(found) == 1, (name, found)
        k[name] = int(found[0])
    assert len(re.findall(r"\bPART_SIZE = 1 << PART_SHIFT\b", text)) == 1
    assert len(re.findall(r"\bPART_MAX_N = \(int64_t\)PART_MAX << PART_SHIFT;", text)) == 1
    k["PART_SIZE"] = 1 << k["PART_SHIFT"]
    k["PART_MAX_N"] = k["PART_MAX"] << k["PART_SHIFT"]
    found = re.findall(r"return n > (\d+) \* PART_SIZE && n <= PART_MAX_N;", text)
    assert len(found) == 1, found
    k["PART_ENTER"] = int(found[0])
    found = re.findall(r"__launch_bounds__\((\d+)\) k_part_scan_rows\(", text)
    turns = re.findall(r"for \(int base = 0; base < nwg; base \+= (\d+)\)", text)
    assert len(found) == 1 and found == turns, (found, turns)
    k["SCAN_TURN"] = int(found[0])
    found = re.findall(r"count >= 1 && count <= (\d+) && seeds", text)
    assert len(found) == 1, found
    k["CALL_MAX"] = int(found[0])
    return k


EXPECTED_CONSTANTS = dict(LINK_REG=8, LINK_LDS=24, PART_SHIFT=11, PART_SIZE=2048, PART_MAX=2048, PART_MAX_N=4194304,
                          PART_CHUNK=16384, PART_ENTER=16, SCAN_TURN=1024, CALL_MAX=32)
K = kernel_constants()
FIRST_PART_N = K["PART_ENTER"] * K["PART_SIZE"] + 1   # the smallest n of the partitioned path


def partitioned(n):
    return K["PART_ENTER"] * K["PART_SIZE"] < n <= K["PART_MAX_N"]


def edge_sizes():
    """name -> n, every n made of the parsed constants (tests/test_gpu_randperm.py runs each with three seeds)."""
    size, chunk, turn = K["PART_SIZE"], K["PART_CHUNK"], K["SCAN_TURN"]
    enter = K["PART_ENTER"] * size
    return {
        "last size of the atomic path": enter,
        "first size of the partitioned path": enter + 1,
        "one step into a third counting workgroup": enter + 2,
        "last partition full": (K["PART_ENTER"] + 1) * size,
        "last partition of one position": (K["PART_ENTER"] + 1) * size + 1,
        "last counting workgroup full": 3 * chunk + 1,
        "last counting workgroup with one step": 3 * chunk + 2,
        "second scan turn not entered: SCAN_TURN partitions": turn * size,
        "second scan turn with one entry": turn * size + 1,
        "ragged second scan turn": (3 * turn // 2 - 36) * size - 5,   # a second turn of 476 entries: no multiple of a wave
        "first atomic size past PART_MAX_N": K["PART_MAX_N"] + 1,
    }


EDGE_SEEDS = (3, 19920517, 2 ** 63 - 1)
BATCH_COUNTS = (1, K["CALL_MAX"] - 1, K["CALL_MAX"], K["CALL_MAX"] + 1)   # seeds per ops.randperm call at FIRST_PART_N


# ---------------------------------------------------------------------------------------------------------------------
# (seed, n) pairs that reach each list branch.  Found by a CPU scan over seeds (the longest list of a permutation has
# about ln n entries; one longer than LINK_LDS turns up in roughly one seed in a thousand at these n); the numbers are
# not trusted: test_pairs_reach_their_branches recomputes every census and asserts what each pair is there for.

def _classes(seed, n):
    c = census(seed, n)
    return {"reg": bool(((c >= 1) & (c <= K["LINK_REG"])).any()),
            "lds": bool(((c > K["LINK_REG"]) & (c <= K["LINK_LDS"])).any()),
            "rewalk": bool((c > K["LINK_LDS"]).any())}


def long_positions(seed, n):
    """positions whose list is longer than LINK_LDS"""
    return np.nonzero(census(seed, n) > K["LINK_LDS"])[0]


# partitioned path, by n: rows of (seed, class of the longest list, partition of the lists longer than LINK_LDS).
# "rewalk" = the longest list exceeds LINK_LDS, "lds" = it exceeds LINK_REG but not LINK_LDS; "inner" = every such list
# lies in a partition before the last one, "last" = in the last one.  The long lists sit within a few positions of the
# end, so at n = k * PART_SIZE + 1 (a last partition of one position) most of them are "inner" ones; at
# n = 17 * PART_SIZE they are in a full last partition.
PART_PAIRS = {
    FIRST_PART_N: [(2508, "rewalk", "inner"), (1, "lds", None), (2948, "rewalk", "inner"), (25333, "rewalk", "last")],
    (K["PART_ENTER"] + 1) * K["PART_SIZE"]: [(2, "lds", None), (11846, "rewalk", "last")],
    2 * FIRST_PART_N - 1: [(700, "rewalk", "inner"), (19920517, "lds", None), (1435, "rewalk", "last"), (2864, "rewalk", "inner")],
}

# atomic path (k_links): a list longer than LINK_REG below the partitioned sizes and above them
ATOMIC_PAIRS = [(5, 2049), (19920517, K["PART_ENTER"] * K["PART_SIZE"]), (7, K["PART_MAX_N"] + 1)]


def all_part_pairs():
    return [(seed, n) for n, row in PART_PAIRS.items() for seed, _, _ in row]


# ---------------------------------------------------------------------------------------------------------------------
# the sampler's plans

PLANS = [  # (epochs, val_duration, n, batch size, the epochs after which the reference evaluates)
    (1, 1, 1003, 64, []),                          # a lone epoch: no evaluation pass, one batch of permutations
    (5, 2, 1003, 64, [2, 4]),
    (3, 7, 1003, 64, [3]),                         # val_duration > epochs: every min(7, 3) = 3 epochs
    (4, 1, FIRST_PART_N + 64, 4096, [1, 2, 3, 4]),   # the permutations take the partitioned path
]
PLAN_SEED = 11


@functools.lru_cache(maxsize=None)
def loader_run(epochs, n, bs, evals):
    """A real DataLoader(shuffle=True) consumed as the reference's fit consumes it: one iterator per training epoch,
    and one more after every epoch in `evals`.  Returns the index order of every training epoch and the global
    generator's next int64 draw after the run."""
    from torch.utils.data import DataLoader
    torch.manual_seed(PLAN_SEED)
    loader = DataLoader(range(n), batch_size=bs, shuffle=True)
    orders = []
    for e in range(1, epochs + 1):
        orders.append(torch.cat([b for b in loader]))
        if e in evals:
            for _ in loader:
                pass
    return orders, int(torch.empty((), dtype=torch.int64).random_().item())


# ---------------------------------------------------------------------------------------------------------------------
# CPU tests

@pytest.mark.parametrize("n", [1, 2, 3, 625, 4097])
def test_reference_equals_torch_randperm(n):
    for seed in (0, 5, 19920517, 2 ** 40 + 17, 2 ** 63 - 1):
        want = torch_randperm(seed, n).numpy()
        assert np.array_equal(reference_randperm(seed, n), want), (seed, n)
        assert int(census(seed, n).sum()) == n - 1 and (census(seed, n)[:1] <= 1).all()


def test_issue_checked_formula_cases():
    for seed, n in ((5, 1000), (2 ** 40 + 17, 4097)):
        assert np.array_equal(reference_randperm(seed, n), torch_randperm(seed, n).numpy())


def test_census_counts_the_steps_per_target():
    j = targets(19920517, 4097)
    c = census(19920517, 4097)
    assert len(j) == 4096 and (j >= np.arange(4096)).all() and (j <= 4096).all()
    for p in (0, 1, 2000, 4095, 4096):
        assert c[p] == sum(1 for t in j.tolist() if t == p)


def test_kernel_constants_are_the_ones_the_edges_are_built_from():
    assert K == EXPECTED_CONSTANTS
    assert edge_sizes() == {
        "last size of the atomic path": 32768,
        "first size of the partitioned path": 32769,
        "one step into a third counting workgroup": 32770,
        "last partition full": 17 * 2048,
        "last partition of one position": 17 * 2048 + 1,
        "last counting workgroup full": 16384 * 3 + 1,
        "last counting workgroup with one step": 16384 * 3 + 2,
        "second scan turn not entered: SCAN_TURN partitions": 2097152,
        "second scan turn with one entry": 2097153,
        "ragged second scan turn": 1500 * 2048 - 5,
        "first atomic size past PART_MAX_N": 4194305,
    }
    assert FIRST_PART_N == 32769 and BATCH_COUNTS == (1, 31, 32, 33)
    # ops.randperm splits a seed list into library calls of CALL_MAX seeds
    with open(os.path.join(ROOT, "lbdrn-msic_amd", "lbdrn_hip", "ops.py")) as f:
        ops_text = f.read()
    body = ops_text[ops_text.index("def randperm("):]
    body = body[:body.index("\ndef ", 1)]
    assert re.findall(r"range\(0, len\(seeds\), (\d+)\)", body) == [str(K["CALL_MAX"])]
    assert re.findall(r"seeds\[c0:c0 \+ (\d+)\]", body) == [str(K["CALL_MAX"])]


def test_a_changed_constant_is_noticed():
    with open(KERNEL_SOURCE) as f:
        text = f.read()
    for old, new in (("LINK_LDS = 24", "LINK_LDS = 28"), ("LINK_REG = 8", "LINK_REG = 4"), ("PART_SHIFT = 11", "PART_SHIFT = 12"),
                     ("PART_MAX = 2048", "PART_MAX = 4096"), ("PART_CHUNK = 16384", "PART_CHUNK = 8192"),
                     ("n > 16 * PART_SIZE", "n > 32 * PART_SIZE")):
        assert text.count(old) == 1, old
        assert kernel_constants(text.replace(old, new)) != EXPECTED_CONSTANTS, old


def test_edge_sizes_are_the_edges_they_are_named_after():
    e = edge_sizes()
    size, chunk, turn = K["PART_SIZE"], K["PART_CHUNK"], K["SCAN_TURN"]
    npart = lambda n: (n + size - 1) // size                    # noqa: E731  (as carve_perm / randperm_batch count them)
    nwg = lambda n: (n - 1 + chunk - 1) // chunk                # noqa: E731  (workgroups of the counting pass: over the n - 1 steps)
    last_wg_steps = lambda n: (n - 1) - (nwg(n) - 1) * chunk    # noqa: E731
    last_part_positions = lambda n: n - (npart(n) - 1) * size   # noqa: E731
    assert not partitioned(e["last size of the atomic path"]) and partitioned(e["last size of the atomic path"] + 1)
    n = e["first size of the partitioned path"]
    assert partitioned(n) and nwg(n) == 2 and last_wg_steps(n) == chunk and last_part_positions(n) == 1
    n = e["one step into a third counting workgroup"]
    assert partitioned(n) and nwg(n) == 3 and last_wg_steps(n) == 1
    n = e["last partition full"]
    assert partitioned(n) and last_part_positions(n) == size and npart(n) == K["PART_ENTER"] + 1
    n = e["last partition of one position"]
    assert partitioned(n) and last_part_positions(n) == 1 and npart(n) == K["PART_ENTER"] + 2
    n = e["last counting workgroup full"]
    assert partitioned(n) and nwg(n) == 3 and last_wg_steps(n) == chunk
    n = e["last counting workgroup with one step"]
    assert partitioned(n) and nwg(n) == 4 and last_wg_steps(n) == 1
    n = e["second scan turn not entered: SCAN_TURN partitions"]
    assert partitioned(n) and npart(n) == turn
    n = e["second scan turn with one entry"]
    assert partitioned(n) and npart(n) == turn + 1
    n = e["ragged second scan turn"]
    assert partitioned(n) and turn + 1 < npart(n) < 2 * turn and npart(n) % 64 != 0 and nwg(n) < turn
    n = e["first atomic size past PART_MAX_N"]
    assert not partitioned(n) and partitioned(n - 1) and npart(n - 1) == K["PART_MAX"] == 2 * turn
    assert len(set(e.values())) == len(e)


def test_pairs_reach_their_branches():
    reg, lds = K["LINK_REG"], K["LINK_LDS"]
    rewalk_pairs, where_seen = 0, set()
    for n, row in PART_PAIRS.items():
        assert partitioned(n), n
        wants = [want for _, want, _ in row]
        assert "rewalk" in wants and "lds" in wants, n   # permutations that share a launch take different branches
        last_part = (n - 1) >> K["PART_SHIFT"]
        for seed, want, where in row:
            longest = int(census(seed, n).max())
            cl = _classes(seed, n)
            if want == "rewalk":
                assert longest > lds, (seed, n, longest)
                assert cl == {"reg": True, "lds": True, "rewalk": True}, (seed, n, cl)   # all three classes in one permutation
                parts = set((long_positions(seed, n) >> K["PART_SHIFT"]).tolist())
                assert parts and all((p == last_part) == (where == "last") for p in parts), (seed, n, parts, last_part)
                rewalk_pairs += 1
                where_seen.add(where)
            else:
                assert reg < longest <= lds and where is None, (seed, n, longest)
                assert cl == {"reg": True, "lds": True, "rewalk": False}, (seed, n, cl)
    assert rewalk_pairs >= 2 and where_seen == {"inner", "last"}
    for seed, n in ATOMIC_PAIRS:
        assert not partitioned(n) and int(census(seed, n).max()) > reg, (seed, n)
        assert bool((census(seed, n) <= reg).any())
    assert any(n <= K["PART_ENTER"] * K["PART_SIZE"] for _, n in ATOMIC_PAIRS)
    assert any(n > K["PART_MAX_N"] for _, n in ATOMIC_PAIRS)


@pytest.mark.parametrize("epochs,val,n,bs,evals", PLANS)
def test_plan_and_seed_draws_replay_the_loader(epochs, val, n, bs, evals):
    from lbdrn_hip import sampler
    plan = sampler.epoch_plan(epochs, val)
    want_plan = []
    for e in range(1, epochs + 1):
        want_plan.append(("train", e))
        if e in evals:
            want_plan.append(("eval", e))
    assert plan == want_plan
    orders, after = loader_run(epochs, n, bs, tuple(evals))
    torch.manual_seed(PLAN_SEED)
    seeds = sampler.draw_pass_seeds(plan)
    assert len(seeds) == epochs
    assert int(torch.empty((), dtype=torch.int64).random_().item()) == after   # the generator stands where the loader left it
    for e in range(epochs):
        assert torch.equal(sampler.permutation(seeds[e], n), orders[e]), e
