"""The LBB3 payload restated from the format text of include/lbdrn_plane3.h: a sequential numpy / Python encoder and
decoder, written from that description and not from csrc/plane3.hip or csrc/plane3.inc.  TEST INFRASTRUCTURE: the host
build of the format text (tests/plane3_host_shim.cpp) and the kernels are compared with it byte for byte.

What is vectorised here is only what the format leaves independent: the 64 rows of a pass (one per lane).  Units, passes,
bands, the columns of a row and the steps of a pass are walked in the order the header gives."""
import numpy as np

T = 64                      # columns of a unit = rows of a pass = lanes
WRITER_S = 256              # rows of a unit as the package's writer cuts them
MAGIC = b"LBP3"
HEADER_WORDS = 5
MAX_C = 16
MAX_SIDE = 1 << 20
Q_ESC = 15
MODES_PER_WORD = 10


class Damaged(ValueError):
    pass


# ---------------------------------------------------------------- geometry

def geometry(C, H, W, S):
    if not (1 <= C <= MAX_C and 1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
        raise ValueError(f"geometry {C} x {H} x {W} is out of range (1..{MAX_C} bands)")
    if S < T or S % T or S > MAX_SIDE:
        raise ValueError(f"S = {S} is not a multiple of 64 in 64..2^20")
    return -(-W // T), -(-H // S)       # TX, NU


def units_of(C, H, W, S):
    """(x0, y0, tw, uh) of every unit in table order: rows of units top to bottom, units left to right within a row"""
    TX, NU = geometry(C, H, W, S)
    return [(T * ux, S * uy, min(T, W - T * ux), min(S, H - S * uy)) for uy in range(NU) for ux in range(TX)]


def mode_words(C):
    return -(-C // MODES_PER_WORD)


def min_unit_words(C, uh):
    return C + -(-uh // T) * mode_words(C) + 1


def max_unit_words(C, uh, tw):
    """a lane takes at most one word a symbol"""
    NP = -(-uh // T)
    return C + NP * mode_words(C) + C * uh * tw


# ---------------------------------------------------------------- predictors (a left, b up, d up-left; int64 arrays)

def inner(a, b, d, m):
    if m == 0:
        mn, mx = np.minimum(a, b), np.maximum(a, b)
        return np.where(d >= mx, mn, np.where(d <= mn, mx, a + b - d))
    if m == 1:
        return (a + b) >> 1
    if m == 2:
        return a + b - d
    return ((3 * (a + b) - 2 * d + (1 << 20)) >> 2) - (1 << 18)


def predict_window(win, first_pass, m):
    """win: [rows + 1, tw + 1] int64, the pass's pixels with the row above in row 0 and a column of zeros in column 0.
    The prediction of every pixel of the pass under spatial predictor m, with the unit's border rules."""
    a, b, d = win[1:, :-1], win[:-1, 1:], win[:-1, :-1]
    pred = inner(a, b, d, m)
    pred[:, 0] = b[:, 0]                 # first column of the unit: from above only
    if first_pass:
        pred[0, :] = a[0, :]             # first row of the unit: from the left only (its first pixel: 0, the padding)
    return pred


def fold(e):
    e = ((np.asarray(e, np.int64) + 32768) & 0xFFFF) - 32768        # modulo 2^16, as a signed 16-bit number
    return np.where(e >= 0, 2 * e, -2 * e - 1)


def unfold(v):
    v = np.asarray(v, np.int64)
    return np.where(v & 1, -((v + 1) >> 1), v >> 1)


def residuals(win, prev, first_pass, mode):
    """raw x - prediction of the pass under mode 0..7 (not yet reduced modulo 2^16)"""
    m = mode & 3
    e = win[1:, 1:] - predict_window(win, first_pass, m)
    if mode >= 4:
        e = e - (prev[1:, 1:] - predict_window(prev, first_pass, m))
    return e


# ---------------------------------------------------------------- the lane coder's state (arrays over the lanes)

def rice_k(A, N):
    k = np.zeros(A.shape, np.int64)
    for _ in range(15):
        k = k + ((k < 15) & ((N << (k + 1)) < A))
    return k


def group_size(A, N):
    return np.where(16 * A < N, 16, np.where(2 * A < N, 4, 1))


def update(A, N, v):
    A = A + v
    N = N + 1
    wrap = N == 32
    return np.where(wrap, (A + 1) >> 1, A), np.where(wrap, 16, N)


def initial_state(k0, z0, n):
    a = 0 if z0 == 2 else (1 if z0 == 1 else 6 << k0)
    return np.full(n, a, np.int64), np.full(n, 4, np.int64)


def start_parameters(best, count):
    """what the writer puts into a band's head word: from the band's smallest residual sum over the unit's first pass"""
    k0 = 0
    while k0 < 15 and (count << (k0 + 1)) < best:
        k0 += 1
    z0 = 2 if 16 * best < count else (1 if 2 * best < count else 0)
    return k0, z0


# ---------------------------------------------------------------- encoder

def _code_rows(v, A, N):
    """v: [rows, tw] folded residuals, one row a lane.  -> (code, length) of every symbol and the lanes' state behind."""
    rows, tw = v.shape
    zrun = np.zeros((rows, tw + 1), np.int64)          # zeros in a row from column j on
    for j in range(tw - 1, -1, -1):
        zrun[:, j] = np.where(v[:, j] == 0, zrun[:, j + 1] + 1, 0)
    code = np.zeros((rows, tw), np.uint64)
    length = np.zeros((rows, tw), np.int64)
    left = np.zeros(rows, np.int64)
    zero = np.zeros(rows, bool)
    for j in range(tw):
        x = v[:, j]
        start = left == 0
        g = np.minimum(group_size(A, N), tw - j)
        flagged = start & (group_size(A, N) > 1)
        all0 = zrun[:, j] >= g
        zero = np.where(start, flagged & all0, zero)
        left = np.where(start, g, left)
        c = np.where(flagged & ~all0, 1, 0).astype(np.uint64)
        n = flagged.astype(np.int64)
        k = rice_k(A, N)
        q = x >> k
        esc = q >= Q_ESC
        sym_len = np.where(esc, 31, q + 1 + k)
        qq = np.where(esc, 0, q)
        sym = np.where(esc, (0x7FFF << 16) | x, (((1 << qq) - 1) << (k + 1)) | (x & ((1 << k) - 1))).astype(np.uint64)
        coded = ~zero
        c = np.where(coded, (c << np.where(coded, sym_len, 0).astype(np.uint64)) | sym, c)
        n = n + np.where(coded, sym_len, 0)
        code[:, j], length[:, j] = c, n
        left = left - 1
        A, N = update(A, N, x)
    return code, length, A, N


def _bits_to_words(code, length):
    """one lane's symbols -> its stream as 32-bit words, MSB first, zero padded; at least one word"""
    total = int(length.sum())
    if total:
        idx = np.repeat(np.arange(length.size), length)
        first = np.cumsum(length) - length
        off = np.arange(total) - np.repeat(first, length)
        bits = ((code[idx] >> (length[idx] - 1 - off).astype(np.uint64)) & np.uint64(1)).astype(np.uint8)
    else:
        bits = np.zeros(0, np.uint8)
    nwords = total // 32 + 1
    padded = np.zeros(32 * nwords, np.uint8)
    padded[:total] = bits
    return np.packbits(padded).view(">u4").astype(np.uint32)


def encode_unit(planes, x0, y0, tw, uh):
    """-> the unit's words (uint32 array)"""
    C = planes.shape[0]
    NP = -(-uh // T)
    lanes = min(uh, T)
    head, modes = [], []
    state = [None] * C
    codes = [[] for _ in range(lanes)]      # per lane: (code, length) arrays in stream order
    sym_lengths = []                        # per (pass, band): [rows, tw]
    for p in range(NP):
        rows = min(T, uh - T * p)
        prev = None
        for c in range(C):
            win = np.zeros((rows + 1, tw + 1), np.int64)
            win[1:, 1:] = planes[c, y0 + T * p: y0 + T * p + rows, x0:x0 + tw]
            if p:
                win[0, 1:] = planes[c, y0 + T * p - 1, x0:x0 + tw]
            best, mode, v = None, 0, None
            for m in range(8 if c else 4):
                f = fold(residuals(win, prev, p == 0, m))
                s = int(f.sum())
                if best is None or s < best:
                    best, mode, v = s, m, f
            modes.append(mode)
            if p == 0:
                k0, z0 = start_parameters(best, rows * tw)
                head.append(k0 | (z0 << 12))
                state[c] = initial_state(k0, z0, lanes)
            A, N = state[c]
            code, length, A2, N2 = _code_rows(v, A[:rows], N[:rows])
            A, N = A.copy(), N.copy()
            A[:rows], N[:rows] = A2, N2
            state[c] = (A, N)
            for i in range(rows):
                codes[i].append((code[i], length[i]))
            sym_lengths.append(length)
            prev = win
    streams = [_bits_to_words(np.concatenate([c for c, _ in codes[i]]), np.concatenate([n for _, n in codes[i]])) for i in range(lanes)]
    # The hand-out.  Before it decodes a symbol, a lane that holds fewer than 32 bits takes the unit's next word.  A symbol is
    # at most 32 bits, so one word a step is enough, and once the lane has decoded the symbol that starts at bit B of its
    # stream it has taken ceil(B / 32) + 1 words.  The lanes that take at one step take in lane order.
    consumed = np.zeros(lanes, np.int64)
    taken = np.zeros(lanes, np.int64)
    out = list(head)
    MW = mode_words(C)
    for p in range(NP):
        rows = min(T, uh - T * p)
        for w in range(MW):
            out.append(sum(modes[p * C + c] << (3 * (c - MODES_PER_WORD * w)) for c in range(MODES_PER_WORD * w, min(C, MODES_PER_WORD * (w + 1)))))
        for c in range(C):
            length = sym_lengths[p * C + c]
            B = consumed[:rows, None] + np.cumsum(length, axis=1) - length
            after = -(-B // 32) + 1
            before = np.concatenate([taken[:rows, None], after[:, :-1]], axis=1)
            i, j = np.nonzero(after > before)
            order = np.lexsort((i, i + j))                  # by step d = i + j, then by lane
            for ii, jj in zip(i[order], j[order]):
                t = after[ii, jj] - 1
                out.append(int(streams[ii][t]) if t < streams[ii].size else 0)
            taken[:rows] = after[:, -1]
            consumed[:rows] += length.sum(axis=1)
    return np.asarray(out, np.uint32)


def encode(planes, S=WRITER_S):
    """[C,H,W] uint16 -> the LBB3 body (bytes): header, table of word counts, units"""
    planes = np.ascontiguousarray(planes).astype(np.int64)
    C, H, W = planes.shape
    units = [encode_unit(planes, *u) for u in units_of(C, H, W, S)]
    head = np.array([int.from_bytes(MAGIC, "little"), C, H, W, S], np.uint32)
    table = np.array([u.size for u in units], np.uint32)
    return np.concatenate([head, table] + units).astype("<u4").tobytes()


# ---------------------------------------------------------------- decoder

def parse(body):
    """-> (C, H, W, S, [word array of every unit]); raises Damaged where the header or the table is not sound"""
    if len(body) % 4 or len(body) < 4 * HEADER_WORDS or body[:4] != MAGIC:
        raise Damaged("not an LBB3 body")
    w = np.frombuffer(body, "<u4").astype(np.int64)
    C, H, W, S = (int(v) for v in w[1:5])
    try:
        units = units_of(C, H, W, S)
    except ValueError as e:
        raise Damaged(str(e))
    if w.size < HEADER_WORDS + len(units):
        raise Damaged("the table overruns the body")
    table = w[HEADER_WORDS:HEADER_WORDS + len(units)]
    if int(table.sum()) != w.size - HEADER_WORDS - len(units):
        raise Damaged("the unit word counts do not add up to the body")
    for n, (x0, y0, tw, uh) in zip(table, units):
        if not min_unit_words(C, uh) <= n <= max_unit_words(C, uh, tw):
            raise Damaged("a unit's word count is outside what its size allows")
    ends = HEADER_WORDS + len(units) + np.cumsum(table)
    return C, H, W, S, [w[e - n:e] for e, n in zip(ends, table)]


def decode_unit(words, C, tw, uh):
    """-> [C, uh, tw] int64; raises Damaged"""
    NP = -(-uh // T)
    lanes = min(uh, T)
    MW = mode_words(C)
    out = np.zeros((C, uh, tw), np.int64)
    A, N = [None] * C, [None] * C
    for c in range(C):
        k0, z0 = int(words[c]) & 0xFF, int(words[c]) >> 12
        if k0 > 15 or z0 > 2 or int(words[c]) & 0xF00:
            raise Damaged("head word")
        A[c], N[c] = initial_state(k0, z0, lanes)
    cur = C
    buf = [0] * lanes                      # per lane: the bits it holds, as (value, count)
    nb = [0] * lanes
    for p in range(NP):
        rows = min(T, uh - T * p)
        if cur + MW > words.size:
            raise Damaged("mode words")
        mw = [int(v) for v in words[cur:cur + MW]]
        cur += MW
        prev = None
        for c in range(C):
            word, at = mw[c // MODES_PER_WORD], 3 * (c % MODES_PER_WORD)
            mode = (word >> at) & 7
            last = min(C, MODES_PER_WORD * (c // MODES_PER_WORD + 1)) - 1
            if (c == 0 and mode >= 4) or (c == last and word >> (at + 3)):
                raise Damaged("mode")
            m = mode & 3
            win = np.zeros((rows + 1, tw + 1), np.int64)
            if p:
                win[0, 1:] = out[c, T * p - 1]
            left = [0] * rows
            zero = [False] * rows
            Ac, Nc = A[c], N[c]
            for d in range(rows + tw - 1):
                for i in range(max(0, d - tw + 1), min(rows, d + 1)):
                    j = d - i
                    if nb[i] < 32:
                        if cur >= words.size:
                            raise Damaged("the unit's words run out")
                        buf[i] = (buf[i] << 32) | int(words[cur])
                        nb[i] += 32
                        cur += 1

                    def take(n, i=i):
                        nb[i] -= n
                        v = buf[i] >> nb[i]
                        buf[i] &= (1 << nb[i]) - 1
                        return v
                    a_, n_ = int(Ac[i]), int(Nc[i])
                    if left[i] == 0:
                        g = 16 if 16 * a_ < n_ else (4 if 2 * a_ < n_ else 1)
                        zero[i] = False
                        if g > 1:
                            g = min(g, tw - j)
                            zero[i] = take(1) == 0
                        left[i] = g
                    v = 0
                    if not zero[i]:
                        k = 0
                        while k < 15 and (n_ << (k + 1)) < a_:
                            k += 1
                        q = 0
                        while q < Q_ESC and nb[i] > 0 and (buf[i] >> (nb[i] - 1)) & 1:
                            take(1)
                            q += 1
                        if q == Q_ESC:
                            if nb[i] < 16:
                                raise Damaged("escape")
                            v = take(16)
                        else:
                            if nb[i] < 1 + k:
                                raise Damaged("symbol")
                            take(1)
                            v = (q << k) | take(k)
                    left[i] -= 1
                    a_ += v
                    n_ += 1
                    if n_ == 32:
                        a_, n_ = (a_ + 1) >> 1, 16
                    Ac[i], Nc[i] = a_, n_
                    # the prediction, from what is decoded so far
                    r = i + 1
                    a, b, dd = win[r, j], win[r - 1, j + 1], win[r - 1, j]

                    def pred_of(wn):
                        a, b, dd = int(wn[r, j]), int(wn[r - 1, j + 1]), int(wn[r - 1, j])
                        if p == 0 and i == 0:
                            return a
                        if j == 0:
                            return b
                        return int(inner(np.int64(a), np.int64(b), np.int64(dd), m))
                    pr = pred_of(win)
                    if mode >= 4:
                        pr += int(prev[r, j + 1]) - pred_of(prev)
                    win[r, j + 1] = (pr + int(unfold(v))) & 0xFFFF
            out[c, T * p:T * p + rows] = win[1:, 1:]
            prev = win
    if cur != words.size:
        raise Damaged("words left over behind the unit")
    return out


def decode(body):
    """the LBB3 body -> [C,H,W] uint16; raises Damaged"""
    C, H, W, S, unit_words = parse(bytes(body))
    out = np.zeros((C, H, W), np.uint16)
    for words, (x0, y0, tw, uh) in zip(unit_words, units_of(C, H, W, S)):
        out[:, y0:y0 + uh, x0:x0 + tw] = decode_unit(words, C, tw, uh)
    return out


# ---------------------------------------------------------------- what the host and the GPU tests share

def cases():
    """(name, [C,H,W] uint16) -- the shapes and contents the byte-identity tests run on"""
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(os.path.dirname(here), "lbdrn-msic_amd"))
    from lbdrn_hip.synth import correlated_tile, synthetic_tile
    rng = np.random.default_rng(31)

    def smooth(C, H, W, top=4000):
        y, x = np.mgrid[0:H, 0:W]
        base = 900 + 7 * x + 5 * y + 40 * np.sin(x / 5.0) * np.cos(y / 7.0)
        return np.stack([np.clip(base * (1 + 0.2 * c) + rng.integers(-3, 4, (H, W)), 0, top * 4) for c in range(C)]).astype(np.uint16)

    out = [("one pixel", np.array([[[40000]]], np.uint16)),
           ("one band", smooth(1, 70, 70)),
           ("2x130x1", smooth(2, 130, 1)),
           ("1x1x257", smooth(1, 1, 257)),
           ("3x257x65", smooth(3, 257, 65)),
           ("2x64x64", smooth(2, 64, 64)),
           ("2x65x64", smooth(2, 65, 64)),
           ("16 bands", smooth(16, 70, 66)),
           ("zeros", np.zeros((2, 70, 66), np.uint16)),
           ("constant", np.full((3, 66, 70), 12345, np.uint16)),
           ("noise", rng.integers(0, 65536, (2, 70, 70)).astype(np.uint16))]
    one = smooth(1, 80, 70)
    out.append(("identical bands", np.repeat(one, 4, axis=0)))
    comp = smooth(3, 70, 66)
    comp[1] = 65535 - comp[0]
    comp[2] = 65535 - comp[1]
    out.append(("complement", comp))
    alt = np.zeros((4, 66, 66), np.uint16)
    alt[1::2] = 65535
    out.append(("alternating 0 / 65535", alt))
    spikes = np.zeros((3, 70, 70), np.uint16)
    at = rng.integers(0, 70, (25, 2))
    spikes[1, at[:, 0], at[:, 1]] = rng.integers(1, 65536, 25)
    out.append(("spikes in one band", spikes))
    out.append(("correlated_tile(1, 8, 300, 130) >> 5", correlated_tile(1, 8, 300, 130) >> 5))
    out.append(("synthetic_tile(2, 4, 300, 333) >> 5", synthetic_tile(2, 4, 300, 333) >> 5))
    return out


_bodies = {}


def case_body(name, planes, S=WRITER_S):
    """encode(planes, S), computed once per process"""
    if (name, S) not in _bodies:
        _bodies[(name, S)] = encode(planes, S)
    return _bodies[(name, S)]


def damaged_units():
    """The fixed list of damaged bodies: (name, body, (C, H, W, S)) where the geometry is what the caller states to the decoder.
    Every one must end in a refusal, a status or merely wrong values -- never in an access outside the body or the planes."""
    rng = np.random.default_rng(77)
    y, x = np.mgrid[0:70, 0:66]
    planes = np.stack([np.clip(500 + 9 * x + 4 * y + rng.integers(-20, 21, (70, 66)) + 300 * c, 0, 65535) for c in range(3)]).astype(np.uint16)
    planes[2] = rng.integers(0, 65536, (70, 66))
    C, H, W, S = 3, 70, 66, 64
    geom = (C, H, W, S)
    sound = np.frombuffer(encode(planes, S), "<u4").copy()
    nunits = 4
    table = HEADER_WORDS
    data = HEADER_WORDS + nunits
    out = [("sound", sound.copy(), geom)]

    def variant(name, edit, g=geom):
        w = sound.copy()
        w = edit(w)
        out.append((name, w if w is not None else None, g))

    def setw(i, v):
        def f(w):
            w[i] = v
            return w
        return f
    variant("k0 = 16", setw(data, 16))
    variant("z0 = 3", setw(data + 1, 3 << 12))
    variant("stray head bit", setw(data + 2, sound[data + 2] | 0x100))
    variant("band 0 differential", setw(data + C, sound[data + C] | 4))
    variant("mode bits beyond the bands", setw(data + C, sound[data + C] | (1 << 9)))
    variant("mode word all ones", setw(data + C, 0xFFFFFFFF))

    def shift(w):
        w[table] += 1
        w[table + 1] -= 1
        return w
    variant("a word moved from unit 1 to unit 0", shift)

    def moved(w):
        w[table] -= 100
        w[table + 2] += 100
        return w
    variant("100 words moved from unit 0 to unit 2", moved)

    def smallest(w):
        rest = int(w[table]) - min_unit_words(C, 64)
        w[table] -= rest
        w[table + 3] += rest
        return w
    variant("unit 0 cut to its head", smallest)

    def ones(w):
        w[data + C + 1:data + int(w[table])] = 0xFFFFFFFF
        return w
    variant("unit 0: every taken word all ones", ones)

    def zeros(w):
        w[data + C + 1:data + int(w[table])] = 0
        return w
    variant("unit 0: every taken word zero", zeros)
    variant("a count beyond the body", setw(table + 1, 0xFFFFFFFF))
    variant("every count beyond the body", lambda w: np.concatenate([w[:table], np.full(nunits, 0x7FFFFFFF, np.uint32), w[data:]]))
    variant("zero counts", lambda w: np.concatenate([w[:table], np.zeros(nunits, np.uint32), w[data:]]))
    variant("header says S = 128", setw(4, 128))
    variant("header says another width", setw(3, 67))
    variant("bad magic", setw(0, 0))
    variant("last word missing", lambda w: w[:-1])
    variant("a word too many", lambda w: np.concatenate([w, np.zeros(1, np.uint32)]))
    variant("cut inside the table", lambda w: w[:table + 2])
    variant("cut to the header", lambda w: w[:HEADER_WORDS])
    variant("stated as S = 128", lambda w: w, (C, H, W, 128))
    variant("stated as 16 bands", lambda w: w, (16, H, W, S))
    for t in range(6):
        def flip(w, t=t):
            at = rng.integers(data, w.size, 8)
            w[at] ^= np.uint32(1) << rng.integers(0, 32, 8).astype(np.uint32)
            return w
        variant(f"bit flips {t}", flip)
    return [(name, w.astype("<u4").tobytes(), g) for name, w, g in out]
