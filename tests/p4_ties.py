"""The decision boundaries of p4Bits32 / p4Bits64: the cost model restated on
a histogram of bit widths (cost_table), the boundaries a block sits on
(classes), deliberately wrong variants of the decision (MUTANTS) and one seeded
family of blocks per (fmt, n) in which every boundary the model has at that n
appears in at least QUOTA units (tie_case) -- the inputs of
tests/test_p4_ties_cpu.py and tests/test_gpu_enc_ties.py.

The reference decides serially: from the plain block it walks b downwards,
replaces the running minimum only on a strict improvement and takes the bitmap
patch when psz <= vsz.  In closed form: every b below the block's width is one
candidate of cost min(psz, vsz) and kind bitmap iff psz <= vsz; the winner is
the minimum of (cost, width - b, kind) and the plain block wins equality with
it.  The model reads only the widths of the values, so the search runs over
histograms; values are drawn afterwards.  The one decision that reads values is
vbEnc's raw escape: an exception whose excess over b has 8, 15 or 22 bits has a
vbyte form one byte longer in the upper part of its range ("flex" exceptions,
_FLEX), and a unit records how many of them are drawn there (`high`), which
fixes the exact byte count.  Test infrastructure only."""
import collections
import functools

import numpy as np

import p4_modes
import v32_inputs
import v64_inputs

QUOTA = 8            # units per class and case the tests ask for
FILL = 10            # units per class the search collects
MAX_UNITS = 640
STALL = 5000         # draws without a new unit after which the search ends
EST = (7, 15, 19, 25)  # the estimator's steps: S(b+7) + 2 S(b+15) + 3 S(b+19) + 4 S(b+25)

CASES = [("256v32", 256), ("256v32", 200), ("256v32", 65), ("128v32", 128), ("128v32", 100), ("128v32", 33),
         ("32", 256), ("32", 127), ("32", 33), ("32", 9), ("128v64", 128), ("128v64", 100), ("256v64", 256),
         ("64", 256), ("64", 127)]
FULL_WIDTH32 = [("256v32", 256), ("128v32", 128), ("32", 256), ("32", 127)]
WBITS = {"32": 32, "128v32": 32, "256v32": 32, "64": 64, "128v64": 64, "256v64": 64}
BASE_N = {"32": None, "64": None, "128v32": 128, "256v32": 256, "128v64": 128, "256v64": 128}  # values in the base payload
_FCODE = {"32": 0, "128v32": 1, "256v32": 2, "64": 3, "128v64": 4, "256v64": 5}


def pad8(x):
    return (x + 7) // 8


def block_n(fmt, n):
    """The n of the blocks the planner sees: a 256v64 unit is two 128v64 blocks."""
    return 128 if fmt == "256v64" else n


# ---- vbyte lengths ----------------------------------------------------------------------------
# first value of the 2-, 3- and 4-byte forms (vbPut32 / vbPut64)
_VB_STEP = {32: (156, 16540, 2113692), 64: (152, 16536, 2113688)}
_FLEX = (8, 15, 22)  # excess widths whose range holds one of those steps


def vb_len(x, W):
    """Bytes of one vbEnc32 / vbEnc64 value."""
    s = _VB_STEP[W]
    if x < s[2]:
        return 1 + (x >= s[0]) + (x >= s[1])
    if W == 32:
        return 4 if x <= 0xFFFFFF else 5
    return 1 + pad8(int(x).bit_length())


def vb_len_low(e, W):
    """Bytes of the smallest value of excess width e (e >= 1); a flex width's largest takes one more."""
    return vb_len(1 << (e - 1), W)


# ---- the cost model -----------------------------------------------------------------------------
class Table:
    """cost_table's result.  cnt: the histogram; maxb: the block's width; plain: the plain size; bs, psz, vsz, xc:
    per candidate b = maxb - 1 .. 0 (in the reference's order) the bitmap and vbyte sizes and the exception count;
    b0: the winning width before the 63 -> 64 rule; b, bx: the reference's choice (bx = 0 plain, 1..W bitmap patch
    bits, W + 1 vbyte); kind: "plain", "bitmap" or "vb"; xn: the winner's exceptions."""


def cost_table(widths, n, W, rule=None):
    """widths: cnt[w] = values of width w, w = 0..W, n in all, not all zero and not all equal (the reference tests
    those first, on the values).  rule: a MUTANTS key, for a deliberately wrong decision."""
    cnt = list(widths)
    assert len(cnt) == W + 1 and sum(cnt) == n
    t = Table()
    t.n, t.W, t.cnt = n, W, cnt
    maxb = t.maxb = max(w for w in range(W + 1) if cnt[w])
    assert maxb > 0
    est = tuple(o + (rule == "est_%d" % o) for o in EST)
    S = np.zeros(W + 40, dtype=np.int64)  # S[k]: values wider than k
    S[:W] = np.cumsum(np.asarray(cnt[:0:-1], dtype=np.int64))[::-1]
    t.plain = pad8(n * maxb) + 1
    bs = np.arange(maxb - 1, -1, -1)  # the candidates, in the reference's order
    xc, order = S[bs], maxb - bs
    base = (n * bs + 7) // 8 + 2
    vsz = base + 2 * xc + S[bs + est[0]] + 2 * S[bs + est[1]] + 3 * S[bs + est[2]] + 4 * S[bs + est[3]]
    pbits = xc * order
    psz = base + pad8(n) + (pbits // 8 if rule == "patch_bytes_floor" else (pbits + 7) // 8)
    bitmap = psz < vsz if rule == "vb_wins_equal" else psz <= vsz
    cost, kind = np.where(bitmap, psz, vsz), 1 - bitmap.astype(np.int64)
    if rule == "lowest_b":
        key = (cost << 8) | ((127 - order) << 1) | kind
    elif rule == "kind_over_order":
        key = (cost << 8) | (kind << 7) | order
    else:
        key = (cost << 8) | (order << 1) | kind
    best = int(np.argmin(key))
    t.bs, t.psz, t.vsz, t.xc, t.cost = bs.tolist(), psz.tolist(), vsz.tolist(), xc.tolist(), cost.tolist()
    t.kinds = [("bitmap", "vb")[k] for k in kind.tolist()]
    t.best = best  # index of the best patch candidate
    patch_wins = t.cost[best] <= t.plain if rule == "patch_wins_equal" else t.cost[best] < t.plain
    if patch_wins:
        t.b0, t.kind, t.xn = t.bs[best], t.kinds[best], t.xc[best]
        t.bx = W + 1 if t.kind == "vb" else maxb - t.b0
    else:
        t.b0, t.kind, t.xn, t.bx = maxb, "plain", 0, 0
    t.b = t.b0
    if W == 64 and t.b0 == 63:  # the 63 -> 64 rule: a plain block of 64 bits
        t.b, t.bx, t.kind, t.xn = 64, 0, "plain", 0
    return t


def exc_widths(t, b=None):
    """The excess widths (w - b) of the exceptions over b (default: the winner's), widest first."""
    b = t.b0 if b is None else b
    return [w - b for w in range(t.maxb, b, -1) for _ in range(t.cnt[w])]


def vb_bytes(t, high, b=None):
    """The exact vbEnc byte count of the exceptions over b with `high` of the flex ones in the long half."""
    return sum(vb_len_low(e, t.W) for e in exc_widths(t, b)) + high


def flex_count(t, b=None):
    b = t.b0 if b is None else b
    return sum(t.cnt[b + e] for e in _FLEX if b + e <= t.maxb)


def is_raw(t, high, rule=None):
    """vbEnc's raw escape on the winner's exceptions: op + 32 > out + (W / 8) n."""
    if t.kind != "vb":
        return False
    s, lim = vb_bytes(t, high) + 32, (t.W // 8) * t.xn
    return s >= lim if rule == "raw_escape_ge" else s > lim


def decision(cnt, n, W, high, rule=None):
    """(b, bx, raw) of the reference, or of the mutant `rule`."""
    t = cost_table(cnt, n, W, rule)
    return t.b, t.bx, is_raw(t, min(high, flex_count(t)), rule)


MUTANTS = {
    "lowest_b": "the lowest b wins a tie of costs",
    "vb_wins_equal": "vbyte wins psz == vsz",
    "patch_wins_equal": "a patch wins equality with the plain block",
    "kind_over_order": "among equal costs the kind bit ranks above the order: a bitmap at a lower b beats vbyte at a higher",
    "raw_escape_ge": "the raw escape is taken at equality",
    "est_7": "the estimator's first step at b + 8",
    "est_15": "the estimator's second step at b + 16",
    "est_19": "the estimator's third step at b + 20",
    "est_25": "the estimator's fourth step at b + 26",
    "patch_bytes_floor": "the patch bits' bytes rounded down",
}
# the class whose units a mutant must move
MUTANT_CLASS = {"lowest_b": ("multi_b_bitmap", "multi_b_vb", "multi_b_mixed_hi_bitmap", "multi_b_mixed_hi_vb"),
                "vb_wins_equal": ("bitmap_eq_vb",), "patch_wins_equal": ("plain_eq_patch",),
                "kind_over_order": ("multi_b_mixed_hi_vb",), "raw_escape_ge": ("vb_comp_last",), "est_7": ("est_7",),
                "est_15": ("est_15",), "est_19": ("est_19",), "est_25": ("est_25",), "patch_bytes_floor": ("bitmap_by_1", "bitmap_eq_vb")}

BASE_CLASSES = ("bitmap_eq_vb", "bitmap_by_1", "vb_by_1", "multi_b_bitmap", "multi_b_vb", "multi_b_mixed_hi_bitmap",
                "multi_b_mixed_hi_vb", "plain_eq_patch", "plain_by_1", "patch_by_1", "vb_comp_last", "vb_raw_first", "est_7", "est_15",
                "est_19", "est_25")


def all_classes(W):
    if W == 32:
        return list(BASE_CLASSES)
    return list(BASE_CLASSES) + [c + s for s in ("_x32", "_w64") for c in BASE_CLASSES] + ["quirk63_tied"]


def classes(t, high=0):
    """The boundaries the block of cost_table `t` sits on (high: its flex exceptions in the long half)."""
    out = set()
    i = t.best
    mincost = t.cost[i]
    if t.kind == "plain" and t.b0 == t.maxb:
        if t.plain == mincost:
            out.add("plain_eq_patch")
        if t.plain + 1 == mincost:
            out.add("plain_by_1")
    else:
        if mincost + 1 == t.plain:
            out.add("patch_by_1")
        if t.kinds[i] == "bitmap":
            if t.psz[i] == t.vsz[i]:
                out.add("bitmap_eq_vb")
            if t.psz[i] + 1 == t.vsz[i]:
                out.add("bitmap_by_1")
        else:
            if t.vsz[i] + 1 == t.psz[i]:
                out.add("vb_by_1")
        tied = [j for j in range(len(t.bs)) if t.cost[j] == mincost]
        if len(tied) > 1 and mincost < t.plain:
            kinds = {t.kinds[j] for j in tied}
            if len(kinds) == 1:
                out.add("multi_b_" + t.kinds[i])
            else:
                out.add("multi_b_mixed_hi_" + t.kinds[i])  # the highest b of the tied is the winner
            if t.W == 64 and t.b0 == 63:
                out.add("quirk63_tied")
        if t.kind == "vb":  # not under the 63 -> 64 rule, which writes no exceptions
            s, lim = vb_bytes(t, high) + 32, (t.W // 8) * t.xc[i]
            if s == lim:
                out.add("vb_comp_last")
            if s == lim + 1:
                out.add("vb_raw_first")
        if t.kinds[i] == "vb":
            for o in EST:
                if t.b0 + o + 1 <= t.maxb and t.cnt[t.b0 + o] and t.cnt[t.b0 + o + 1]:
                    out.add("est_%d" % o)
    if t.W == 64:
        b = t.bs[i]  # the best patch: its exceptions
        base = [c for c in out if c != "quirk63_tied"]
        if t.maxb > 32:
            out.update(c + "_x32" for c in base)
        if t.cnt[64] and b < 64:
            out.update(c + "_w64" for c in base)
    return out


# ---- exemptions ---------------------------------------------------------------------------------
def est_bytes(e):
    """The estimator's price of one vbyte exception of excess width e, without its position byte."""
    return 1 + (e >= 8) + 2 * (e >= 16) + 3 * (e >= 20) + 4 * (e >= 26)


def vbyte_can_win(W, n, need):
    """A NECESSARY condition for a vbyte winner whose exceptions include the excess widths `need`: at the winner's b,
    vsz < psz, that is xn + sum of est_bytes < pad8(n) + pad8(xn * emax).  Given xn and the widest excess emax, the
    cheapest exception set is `need`, the widest one and one-byte exceptions besides, so the enumeration of (xn,
    emax) is complete.  False proves that no block of n values has such a winner."""
    for xn in range(len(need), n):
        for emax in range(max(need), W + 1):
            req = list(need) + ([emax] if emax > max(need) else [])
            if len(req) > xn:
                continue
            vs = xn + sum(est_bytes(e) for e in req) + (xn - len(req))
            if vs < pad8(n) + pad8(xn * emax):
                return True
    return False


_EST_ARG = ("enumeration: of the 350,343,532 multisets of 9 widths 0..32 with two or more distinct widths, taken through orc_p4bits32, "
            "33,915,395 choose vbyte and none of those has exceptions of width b + o and b + o + 1 for o = 7, 15, 19 or 25 "
            "(for o = 19 and 25 vbyte_can_win(32, 9, (o, o + 1)) is False as well: the bitmap patch is never dearer)")
_RAW_ARG = "sumlen + 32 >= 4 xn needs sumlen >= xn, so xn >= 11 exceptions, and a block of 9 values has at most 8"
# (W, block n) -> {class: how it was established}.  Nothing is exempt at the full-width 32-bit cases, nor at any
# 64-bit case; test_p4_ties_cpu.py repeats the arithmetic.
EXEMPT = {(32, 9): {"vb_comp_last": _RAW_ARG, "vb_raw_first": _RAW_ARG, "est_7": _EST_ARG, "est_15": _EST_ARG, "est_19": _EST_ARG,
                    "est_25": _EST_ARG}}


# ---- the search over histograms -----------------------------------------------------------------
def _base_hist(rng, n, W, b0):
    """n values below 2^b0, uniform: half of them b0 bits wide, a quarter b0 - 1, ..."""
    cnt = [0] * (W + 1)
    if b0 == 0:
        cnt[0] = n
        return cnt
    w = b0 - np.minimum(rng.geometric(0.5, size=n) - 1, b0)
    for x in w:
        cnt[int(x)] += 1
    return cnt


def _directed_hist(rng, n, W, shape):
    """Shape 10: a bitmap at b1 tied with vbyte at b1 - 1 -- a few exceptions 20 and more bits over b1, which vbyte
    prices at 7 or 11 bytes each and the bitmap at their width, and about n / 16 values of width exactly b1, which
    one bit less of base pays for as 2-byte vbyte exceptions.  Shapes 11, 12: a few exceptions on either side of an
    estimator step over a base of one width."""
    cnt = [0] * (W + 1)
    if shape == 10:
        if W < 24:
            return None
        b1 = int(rng.integers(1, W - 20))
        x1 = int(rng.integers(1, 9))
        for _ in range(x1):
            cnt[int(rng.integers(b1 + 20, W + 1))] += 1
        per_bit = pad8(n * b1) - pad8(n * (b1 - 1))
        c = max(1, per_bit // 2 + int(rng.integers(-3, 3)))
        cnt[b1] += c
        rest = n - x1 - c
        if rest < 1:
            return None
        lo = _base_hist(rng, rest, W, b1 - 1)
        return [a + c for a, c in zip(cnt, lo)]
    o = int(rng.choice(EST))
    if o + 1 > W:
        return None
    b = int(rng.integers(0, W - o))
    x = 0
    for w, hi in ((b + o, 4), (b + o + 1, 4)):
        k = int(rng.integers(1, hi if shape == 11 else 2))
        cnt[w] += k
        x += k
    if shape == 12:
        for _ in range(2):  # one-byte exceptions of two widths: they keep b below the step's widths at small n
            k = int(rng.integers(0, max(2, n // 4)))
            cnt[min(W, b + int(rng.choice([1, 2, 3, 4, 5, 6, 6, 7, 7, 7])))] += k
            x += k
    if n - x < 1:
        return None
    lo = _base_hist(rng, n - x, W, b)
    return [a + c for a, c in zip(cnt, lo)]


NSHAPES = 13


def _draw_hist(rng, n, W, shape):
    """_draw_shape's histogram; at W = 64 two draws in five get one value of width 64 in place of a zero or a one."""
    cnt = _draw_shape(rng, n, W, shape)
    if cnt is not None and W == 64 and cnt[64] == 0 and cnt[0] + cnt[1] > 2 and rng.random() < 0.4:
        cnt[0 if cnt[0] > 1 else 1] -= 1
        cnt[64] += 1
    return cnt


def _draw_shape(rng, n, W, shape):
    """A base of random width and one to three exception tiers of random width and count, or a directed shape."""
    b0 = int(rng.integers(0, W - 1))
    if shape >= 10:
        return _directed_hist(rng, n, W, shape)
    if W == 64 and shape >= 7:
        b0 = int(rng.integers(30, 63))
    if W == 64 and shape == 9 and n >= 16:
        # the 63 -> 64 rule under a tie: up to 7 values of width 64 over width 63, or width 63 over 62
        top = int(rng.integers(63, 65))
        cnt = [0] * 65
        per_bit = pad8(n * (top - 1)) - pad8(n * (top - 2))
        k = int(rng.integers(1, per_bit // 2 + 3))
        cnt[top] = k
        cnt[top - 1] = max(1, per_bit // 2 + int(rng.integers(-1, 2)))
        rest = n - cnt[top] - cnt[top - 1]
        if rest <= 0:
            return None
        lo = _base_hist(rng, rest, 64, top - 2 - int(rng.integers(0, 3)))
        return [a + c for a, c in zip(cnt, lo)]
    tiers = int(rng.integers(1, 4))
    ex = []
    left = n - 1
    for _ in range(tiers):
        if left < 1:
            break
        c = int(min(left, np.exp(rng.uniform(0, np.log(max(2, n // 2))))))
        if shape in (3, 4):  # around the raw escape: 11 (W = 64: 5) to 40 exceptions, most one byte long
            c = int(min(left, rng.integers(2, 30)))
        w = int(rng.integers(b0 + 1, W + 1))
        if shape in (3, 4, 5) and b0 + 8 <= W:  # a tier on an estimator or vbyte step
            w = min(W, b0 + int(rng.choice([7, 8, 9, 15, 16, 17, 19, 20, 21, 22, 23, 25, 26, 27])))
        if W == 64 and shape == 8:
            w = 64
        ex.append((w, c))
        left -= c
    nbase = n - sum(c for _, c in ex)
    if nbase < 1:
        return None
    cnt = _base_hist(rng, nbase, W, b0)
    for w, c in ex:
        cnt[w] += c
    if shape in (5, 6) and b0 + 9 <= W:  # one wider neighbour, for the "one bit wider" of the estimator classes
        w, _ = ex[0]
        if w + 1 <= W and cnt[0 if b0 == 0 else b0] > 1:
            cnt[b0] -= 1
            cnt[w + 1] += 1
    return cnt


def _neighbours(rng, cnt, n, W):
    """The histogram and up to eight variants with one value moved between two widths: ties lie next to near-ties."""
    out = [cnt]
    used = [w for w in range(W + 1) if cnt[w]]
    for _ in range(8):
        src = int(rng.choice(used))
        dst = int(min(W, max(0, src + int(rng.choice([-2, -1, 1, 2, 7, 8])))) if rng.random() < 0.5 else int(rng.choice(used)))
        if src == dst:
            continue
        c = list(cnt)
        c[src] -= 1
        c[dst] += 1
        out.append(c)
    return out


def _highs(t, rng):
    """The `high` values worth trying for a table: the two sides of the raw escape where the flex exceptions reach
    them, and a random one."""
    if t.kind != "vb":
        return [0]
    nf = flex_count(t)
    need = (t.W // 8) * t.xn - 32 - vb_bytes(t, 0)
    out = [int(rng.integers(0, nf + 1))]
    out += [h for h in (need, need + 1) if 0 <= h <= nf]
    return out


@functools.lru_cache(maxsize=None)
def search(W, n, draws=40000):
    """-> (units, counts): units = [(cnt, high, classes)], at most MAX_UNITS, taken greedily from seeded draws while
    some class (or some mutant's kill count) they hold is below FILL; counts: units per class.  The shape of a draw
    is chosen in proportion to the units it has given to the classes still short."""
    rng = np.random.default_rng([9100, W, n])
    ex = EXEMPT.get((W, n), {})
    want = [c for c in all_classes(W) if c not in ex] + ["kill:" + m for m in MUTANTS if not all(c in ex for c in MUTANT_CLASS[m])]
    score = collections.Counter()
    weights = np.ones(NSHAPES)
    have = collections.Counter()
    units, seen = [], set()
    last = 0
    for it in range(draws):
        if it % 100 == 0 and (all(have[c] >= FILL for c in want) or it - last > STALL):
            break
        if it % 50 == 0:
            short = [c for c in want if have[c] < FILL]
            weights = np.array([1.0 + 10.0 * sum(score[sh, c] for c in short) / max(1, len(short)) for sh in range(NSHAPES)])
        shape = int(rng.choice(NSHAPES, p=weights / weights.sum()))
        cnt = _draw_hist(rng, n, W, shape)
        if cnt is None or sum(1 for x in cnt if x) < 2:
            continue
        for c in _neighbours(rng, cnt, n, W):
            if sum(1 for x in c if x) < 2:
                continue
            t = cost_table(c, n, W)
            for high in _highs(t, rng):
                key = (tuple(c), high)
                if key in seen:
                    continue
                cl = classes(t, high)
                if not cl:
                    continue
                ref = (t.b, t.bx, is_raw(t, high))
                tags = set(cl)
                tags |= {"kill:" + m for m in MUTANTS if have["kill:" + m] < FILL and decision(c, n, W, high, m) != ref}
                if any(have[x] < FILL for x in tags) and len(units) < MAX_UNITS:
                    seen.add(key)
                    last = it
                    score.update((shape, x) for x in tags if have[x] < FILL)
                    units.append((c, high, frozenset(cl)))
                    have.update(tags)
    return units, have


# ---- values -------------------------------------------------------------------------------------
def _bits(rng, k):
    """k random bits (k <= 64)."""
    return (int(rng.integers(0, 1 << 32)) | int(rng.integers(0, 1 << 32)) << 32) & ((1 << k) - 1)


def draw_values(rng, cnt, high, n, W):
    """n values with the histogram cnt in random positions; of the winner's flex exceptions `high` lie in the long
    half of their vbyte form and the rest in the short one."""
    t = cost_table(cnt, n, W)
    b = t.b0 if t.kind == "vb" else None
    dt = np.uint32 if W == 32 else np.uint64
    vals, flex = [], []
    for w in range(W + 1):
        for _ in range(cnt[w]):
            v = 0 if w == 0 else (1 << (w - 1)) | _bits(rng, w - 1)
            if b is not None and w - b in _FLEX:
                flex.append(len(vals))
            vals.append(v)
    if b is not None:
        order = rng.permutation(len(flex))
        for k, j in enumerate(order):
            e = int(vals[flex[j]]).bit_length() - b
            step = _VB_STEP[W][_FLEX.index(e)]
            lo, hi = ((step, 1 << e) if k < high else (1 << (e - 1), step))
            x = int(rng.integers(lo, hi))
            vals[flex[j]] = (x << b) | (vals[flex[j]] & ((1 << b) - 1))
    out = np.array(vals, dtype=dt)
    return out[rng.permutation(n)]


class TieCase:
    """One (fmt, n, d1) family with the oracle's stream of it: nu units; hists[i] / highs[i] / classes[i]: per unit the
    blocks' histograms, flex counts and the union of their classes; gaps (nu, n); vals (the gaps, or with d1 the chained
    list they span from CHAIN_START0); starts; units (vals at the full stride, zero past n); packed / off (the oracle's
    bytes); counts: units per class."""

    def __init__(self, fmt, n, d1):
        self.fmt, self.n, self.d1, self.W = fmt, n, d1, WBITS[fmt]
        W, bn = self.W, block_n(fmt, n)
        found, _ = search(W, bn)
        rng = np.random.default_rng([9200, _FCODE[fmt], n])
        per = n // bn
        order = rng.permutation(len(found))
        blocks = [found[i] for i in order]
        if per == 2:  # pair every block with another, so that either half of a unit holds every class
            blocks = [x for i in range(len(blocks)) for x in (blocks[i], blocks[(i + len(blocks) // 2) % len(blocks)])]
        self.nu = len(blocks) // per
        self.hists = [[blocks[i * per + k][0] for k in range(per)] for i in range(self.nu)]
        self.highs = [[blocks[i * per + k][1] for k in range(per)] for i in range(self.nu)]
        self.classes = [frozenset().union(*(blocks[i * per + k][2] for k in range(per))) for i in range(self.nu)]
        self.gaps = np.stack([np.concatenate([draw_values(rng, h, g, bn, W) for h, g in zip(hs, gs)])
                              for hs, gs in zip(self.hists, self.highs)])
        mod = v32_inputs if W == 32 else v64_inputs
        self.start0 = mod.CHAIN_START0
        self.vals, self.starts = mod.d1_list(self.gaps, self.start0) if d1 else (self.gaps, None)
        self.units = mod.padded(self.vals, fmt) if fmt in mod.WIDTH else self.vals
        self.packed, self.off = mod.oracle_stream(fmt, self.units, n, self.starts)
        self.counts = collections.Counter(c for cl in self.classes for c in cl)

    def blocks(self):
        """Every block of the stream, in order: (unit, histogram, high, values, parsed_header's pair, bitmap bx); the
        parse of a unit ends at the next offset."""
        out = []
        bn = block_n(self.fmt, self.n)
        for i in range(self.nu):
            p = int(self.off[i])
            for k in range(self.n // bn):
                hdr, bx, p = parsed_header(self.packed, p, bn, self.W, BASE_N[self.fmt])
                out.append((i, self.hists[i][k], self.highs[i][k], self.gaps[i, k * bn: (k + 1) * bn], hdr, bx))
            assert p == int(self.off[i + 1]), (self.fmt, self.n, i)
        return out

    def names(self, units):
        """For a failure's message: the classes of the first few of `units`."""
        return [(int(u), sorted(self.classes[int(u)])) for u in list(units)[:5]]

    def units_of_bytes(self, bad):
        """The units that hold the byte positions `bad` of the stream."""
        return np.unique(np.searchsorted(self.off, np.asarray(bad, dtype=np.uint64), side="right") - 1)


@functools.lru_cache(maxsize=None)
def tie_case(fmt, n, d1):
    """Cached: callers leave the arrays unchanged."""
    return TieCase(fmt, n, d1)


def np_widths(vals):
    """Bit widths of an array of unsigned values."""
    v = np.asarray(vals).astype(np.uint64)
    w = np.zeros(v.shape, dtype=np.int64)
    for k in range(64):
        w += (v >> np.uint64(k)) != 0
    return w


def choose(values, W):
    """(b, bx, raw) of the reference for a block's values: the all-zero and the constant block first, as p4Bits
    tests them, then cost_table on the widths and the exact vbyte byte count."""
    vals = [int(x) for x in values]
    if not any(vals):
        return 0, 0, False
    if all(v == vals[0] for v in vals):
        return vals[0].bit_length(), W + 2, False
    t = cost_table(np.bincount(np_widths(values), minlength=W + 1).tolist(), len(vals), W)
    raw = False
    if t.kind == "vb":
        raw = sum(vb_len(v >> t.b0, W) for v in vals if v.bit_length() > t.b0) + 32 > (W // 8) * t.xn
    return t.b, t.bx, raw


def header_of(b, bx, raw, W):
    """(header width field, mode) of the block the reference writes for a choice; mode: "plain" (the all-zero block
    included), "const", "bitmap", "vb_raw" or "vb_comp"."""
    hb = 63 if b == 64 else b
    return hb, "plain" if bx == 0 else "const" if bx == W + 2 else ("vb_raw" if raw else "vb_comp") if bx == W + 1 else "bitmap"


_MODE = {"zero": "plain", "plain32": "plain", "plain63": "plain", "const32": "const", "const63": "const"}


def parsed_header(packed, pos, n, W, base_n):
    """header_of's pair, read from a block's bytes with p4_modes; -> (pair, bx byte of a bitmap block or None, end)"""
    if W == 32:
        mode, _, end = p4_modes.parse32(packed, pos, n, base_n)
        bx = int(packed[pos + 1]) if mode == "bitmap" else None
        return (int(packed[pos]) & 0x3F, _MODE.get(mode, mode)), bx, end
    blk = p4_modes.parse64(packed, pos, n, base_n)
    return (blk.b, _MODE.get(blk.mode, blk.mode)), (blk.bx if blk.mode == "bitmap" else None), blk.end


def exempt(fmt, n):
    return EXEMPT.get((WBITS[fmt], block_n(fmt, n)), {})


def required_classes(fmt, n):
    ex = exempt(fmt, n)
    return [c for c in all_classes(WBITS[fmt]) if c not in ex]
