"""The nine running float sums of ppp_trans2center (k_seq_sum, csrc/ppp_preproc.h) on crafted sequences.

pcl::compute3DCentroid and pcl::computeCovarianceMatrix add in float, point after point, and ppp_trans2center promises those
sums bit for bit.  k_seq_sum keeps the promise by turning the additions inside one binade into integer increments of the
mantissa (one increment for an even, one for an odd running mantissa: round half to even), composing them with wave scans, and
adding for real the first value that leaves the binade; after a short stretch it adds a run of values one by one; a sum with no
binade to work in (zero, tiny, inf) is added one value at a time.  The plates of the rest of the suite never steer it to where
these decisions are made.  The sequences here do.

How a test sees a sum.  A handle with change_range = 0 takes the floats as they are.  X is a ramp over 120 mm (it feeds the
plan, and is checked like the rest); Y and Z carry two independent crafted sequences per launch.  The centroid is
sum / float(finite count): every cloud is padded with non-finite points until its finite count is a power of two, so the
division is exact (asserted on the CPU) and a sum that is one ulp off is a centroid that is one ulp off.  A padding point is
+0 inside the sequence for the kernel and absent for the reference; the last point is always finite and non-zero.  The six
covariance sums come back raw and are compared with numpy products in float32 from the returned centroid, in
computeCovarianceMatrix's operand order.  The reference of a sum is np.add.accumulate(v, dtype=np.float32)[-1] over the finite
points; the oracle's trans2center is compared as well.  trim is 1e38 so that the waypoint bound of the plan (y extent over
path_resolution) does not refuse a cloud for its Y values; nothing here plans a path.

Denormals are out of scope: no workpiece in metres or millimetres reaches them.  The tiny family uses normal floats only, and
the CPU tests assert that no product and no partial sum of any case is a non-zero denormal.

The CPU tests take a census of every sequence (ties by parity, binade changes, landings on powers of two, returns to zero,
absorbed values, values of 2^26 ulps or more, steps without a binade, quiet stretches), independent of the kernel, and assert
for every family the counts that make it that family; and that the oracle equals the numpy accumulation bit for bit."""
import numpy as np
import pytest

TILE = 8192          # ppp_preproc.h: SEQ_TILE = SEQ_WAVES * SEQ_CHUNK, the values of one step of a workgroup
SERIAL_BELOW = 2048  # ppp_preproc.h: SEQ_SERIAL_BELOW, a stretch shorter than this is followed by a serial run
SERIAL_RUN = 4096    # ppp_preproc.h: SEQ_SERIAL_RUN, the length of that run (it ends with the tile)
LOW_E = 24           # k_seq_sum: a sum whose exponent field is below 24 (or 255) is added one value at a time
TRIM = 1.0e38
SWEEP_SEED, SWEEP_COUNT = 20261018, 100
LENGTHS = (1, 2, 7, 8, 9, 511, 512, 513, 8191, 8192, 8193, 16389, 24577)
GAPS = (2046, 2047, 2048, 2049)
TAILS = (63, 64, 65, 127, 128, 129, 130)     # values a serial run has left to the end of its tile (130: (b + 1) & 3 == 2)

f32 = np.float32


def ulp(s):
    return np.spacing(np.abs(f32(s)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------- census: exact, independent of the kernel


def census(v):
    """Counts over the sequential float32 accumulation of v (as the kernel sees it: padding as +0).  Everything is decided
    in exact arithmetic: a float32 divided by a power of two is exact in float64, and so are floor and the fraction of it."""
    v = np.ascontiguousarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = np.add.accumulate(v, dtype=np.float32)
    prev = np.concatenate([np.zeros(1, np.float32), acc[:-1]])
    bp, ba = bits(prev), bits(acc)
    Ep, Ea = ((bp >> 23) & 0xff).astype(np.int64), ((ba >> 23) & 0xff).astype(np.int64)
    binade = (Ep >= LOW_E) & (Ep < 255)                      # the running sum has a binade the kernel works in
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        q = v.astype(np.float64) / np.ldexp(1.0, np.maximum(Ep, 1) - 150)      # the value in ulps of the running sum
        frac = q - np.floor(q)
    half = binade & np.isfinite(q) & (frac == 0.5)
    stays = Ea == Ep
    odd = (bp & 1) == 1
    pow2 = ((ba & 0x7fffff) == 0) & (Ea >= 1) & (Ea < 255) & (ba != bp) & ((ba >> 31) == (bp >> 31))
    up = binade & pow2 & (Ea == Ep + 1)                      # 2^24 ulps, from below
    bottom = binade & pow2 & stays                           # 2^23 ulps, from above
    big = binade & ~(np.abs(q) < 2.0 ** 26)
    viol = ~binade | ~stays | bottom | big                   # not a quiet step inside one binade
    at = np.nonzero(viol)[0]
    return dict(
        acc=acc, viol=at, stretches=np.diff(at) - 1,
        ties_even=int((half & stays & ~odd).sum()), ties_odd=int((half & stays & odd).sum()),
        binade_changes=int((Ea != Ep).sum()), changes_at=np.nonzero(Ea != Ep)[0],
        up=int(up.sum()), up_tie=int((up & half).sum()), up_exact=int((up & (frac == 0)).sum()),
        up_rounded=int((up & ~half & (frac != 0)).sum()),
        bottom=int(bottom.sum()), bottom_exact=int((bottom & (frac == 0)).sum()), bottom_rounded=int((bottom & (frac != 0)).sum()),
        below_bottom=int((binade & (Ea == Ep - 1) & (np.abs(q) < 4) & (frac != 0)).sum()),
        zero_returns=int(((acc == 0) & (prev != 0)).sum()),
        absorbed=int(((v != 0) & (ba == bp)).sum()),
        big=int(big.sum()), near_big=int((binade & (np.abs(q) >= 2.0 ** 25) & (np.abs(q) < 2.0 ** 26)).sum()),
        low_e=int((Ep < LOW_E).sum()), first_nonzero=int(np.nonzero(v)[0][0]) if v.any() else len(v),
        negative_steps=int((prev < 0).sum()))


# ---------------------------------------------------------------- building a sequence


QUIET = (0.25, -0.25, 0.5, -0.5, 0.75, -0.75, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0, 3.0, -3.0)
WHOLE = (1.0, -1.0, 2.0, -2.0, 3.0, -3.0)
TIES = (0.5, -0.5, 1.5, -1.5, 2.5, -2.5)
OTHERS = (1.0, -1.0, 3.0, -3.0, 1.0, -1.0, 0.25, -0.25, 0.75, -0.75, 1.25, -1.25, 2.0, -2.0, 0.3, -0.3, 1.7, -1.7)


def choose_pads(n, rng, reserved=(), finite=None):
    """which points are non-finite: the finite count becomes a power of two; never the last point, never a reserved place"""
    if finite is None:
        finite = 1 << (n.bit_length() - 1)
    cand = np.setdiff1d(np.arange(n - 1), np.asarray(list(reserved), np.int64))
    pad = np.zeros(n, bool)
    if n > finite:
        pad[rng.choice(cand, n - finite, replace=False)] = True
    return pad


class Seq:
    """a sequence as the kernel sees it, written front to back; the places of the padding points stay +0 and are stepped over"""

    def __init__(self, pad, rng):
        self.pad, self.n, self.rng = pad, len(pad), rng
        self.v = np.zeros(self.n, np.float32)
        self.i = 0
        self.s = f32(0)

    def add(self, x):
        while self.pad[self.i]:
            self.i += 1
        x = f32(x)
        self.v[self.i] = x
        self.i += 1
        with np.errstate(over="ignore"):
            self.s = f32(self.s + x)
        return self.i - 1

    def goto(self, target):
        target = f32(target)
        self.add(f32(target - self.s))
        assert self.s == target, (self.s, target)

    def quiet_until(self, end, steps=QUIET):
        """steps of a few ulps of the running sum up to place `end` (not included)"""
        assert self.i <= end <= self.n, (self.i, end)
        pick = self.rng.integers(0, len(steps), max(end - self.i, 1))
        while self.i < end:
            if self.pad[self.i]:
                self.i += 1
            else:
                self.add(f32(steps[pick[end - self.i - 1]]) * ulp(self.s))

    def quiet(self, k, steps=QUIET):
        self.quiet_until(self.i + k, steps)

    def finish(self, steps=WHOLE):
        self.quiet_until(self.n, steps)
        assert self.v[-1] != 0
        return self.v


def ties(pad, rng, sign, u):
    """an odd mantissa (8388609 ulps), up to the middle of the binade, then half-ulp ties and other fractions"""
    q = Seq(pad, rng)
    q.add(sign * 8388609.0 * u)
    q.add(sign * 4194304.0 * u)
    tie = rng.random(q.n) < 0.5
    a, b = rng.integers(0, len(TIES), q.n), rng.integers(0, len(OTHERS), q.n)
    while q.i < q.n:
        if q.pad[q.i]:
            q.i += 1
        else:
            q.add(f32(TIES[a[q.i]] if tie[q.i] else OTHERS[b[q.i]]) * f32(u))
    return q.v


def landings_top(pad, rng, sign, u):
    """2^24 ulps reached from below: by a tie from an odd and from an even mantissa, by an exact increment, by rounding, and
    passed; each time back under it.  4200 quiet values before every landing: the scan, not a serial run, meets it.
    (Whether the kernel treats a landing on exactly 2^24 ulps as leaving the binade or not makes no difference to any sum: from
    there every result at or below 2^24 lies on the old grid, where the integer step is the float step, and every result above
    it leaves the binade in either reading.  What these sequences check is that the landing and the way back are right.)"""
    q = Seq(pad, rng)
    top, s, u = f32(16777216.0 * u), f32(sign), f32(u)
    q.add(s * (top - 4096 * u))
    for kind in range(5):
        q.quiet(4200)
        if kind == 0:
            q.goto(s * (top - 3 * u)); q.add(s * 2.5 * u); assert q.s == s * top; q.add(s * -3 * u)
        elif kind == 1:
            q.goto(s * (top - 3 * u)); q.add(s * 3 * u); assert q.s == s * top; q.add(s * -1 * u)
        elif kind == 2:
            q.goto(s * (top - 2 * u)); q.add(s * 1.75 * u); assert q.s == s * top; q.add(s * -0.5 * u); q.add(s * -1 * u)
        elif kind == 3:
            q.goto(s * (top - 1 * u)); q.add(s * 4 * u); assert q.s == s * (top + 4 * u); q.add(s * -6 * u)
        else:
            q.goto(s * (top - 2 * u)); q.add(s * 1.5 * u); assert q.s == s * top; q.add(s * -2 * u)
        q.goto(s * (top - (4096 + int(rng.integers(0, 64))) * u))
    return q.finish(QUIET)


def landings_bottom(pad, rng, sign, u):
    """2^23 ulps reached from above, exactly and by rounding, and the finer grid below it: half-ulps of the old grid right
    under it, quarter-ulps further down.  The last landing is on 2^23 - 1/2 and the sequence ends below, in whole ulps of the
    finer grid: a sum left on 2^23 there stays half an old ulp off to the end"""
    q = Seq(pad, rng)
    bot, s, u = f32(8388608.0 * u), f32(sign), f32(u)
    q.add(s * (bot + 4096 * u))
    stride = (q.n - 400) // 5
    for j, kind in enumerate((0, 2, 3, 4, 1)):
        q.quiet_until((j + 1) * stride)
        if kind == 0:
            q.goto(s * (bot + 3 * u)); q.add(s * -3 * u); assert q.s == s * bot
            q.add(s * -0.5 * u); q.add(s * -0.75 * u); q.add(s * 0.25 * u)
        elif kind == 1:
            q.goto(s * (bot + 1 * u)); q.add(s * -1.5 * u); assert q.s == s * (bot - 0.5 * u)
        elif kind == 2:
            q.goto(s * (bot + 2 * u)); q.add(s * -2.5 * u); assert q.s == s * (bot - 0.5 * u)
        elif kind == 3:
            q.goto(s * (bot + 1 * u)); q.add(s * -1.375 * u); assert q.s == s * (bot - 0.5 * u)
        else:
            q.goto(s * (bot + 2 * u)); q.add(s * -2.25 * u); assert q.s == s * bot
        if kind != 1:
            q.quiet(40)                                    # on the finer grid
            q.goto(s * (bot / 2 + 1000 * u)); q.goto(s * (bot / 2 - 1000.25 * u)); q.quiet(40)   # quarter-ulps of the old grid
            q.goto(s * (bot / 2 + 1000 * u)); q.goto(s * (bot + (4096 + int(rng.integers(0, 64))) * u))
    q.add(s * -256 * u)                                    # room for the last walk under 2^23
    return q.finish(WHOLE)


def zero_returns(pad, rng, late):
    """a leading run of +0 and -0; then x, -x pairs and x, y, -(x + y) triples, each back to exactly zero; then (not late) a last
    quarter of plain values.  late: nothing but zeros until the last 30 finite places"""
    n = len(pad)
    v = np.zeros(n, np.float32)
    free = np.nonzero(~pad)[0]
    lead = free[: 300 if not late else len(free) - 30]
    v[lead] = np.where(rng.random(len(lead)) < 0.5, f32(0.0), f32(-0.0))
    rest = free[len(lead):]
    x = (np.exp2(rng.uniform(-20, 20, len(rest))) * rng.choice([-1.0, 1.0], len(rest))).astype(np.float32)
    k, stop = 0, len(rest) - 3 if late else 3 * len(rest) // 4
    while k + 2 < stop:
        if rng.random() < 0.7:
            x[k + 1] = -x[k]
            k += 2
        else:
            x[k + 2] = -f32(x[k] + x[k + 1])
            k += 3
    v[rest] = x
    assert v[-1] != 0
    return v


def churn(pad, rng, runs):
    """+-1e6 with small residues inside the runs (almost every addition changes binade), a quiet walk between them"""
    n = len(pad)
    v = rng.normal(0, 30, n).astype(np.float32)
    for a, b in runs:
        idx = np.arange(a, b)[~pad[a:b]]
        v[idx] = (1.0e6 * np.where(np.arange(len(idx)) % 2 == 0, 1.0, -1.0) + rng.uniform(-50, 50, len(idx))).astype(np.float32)
    v[pad] = 0
    assert v[-1] != 0
    return v


def stretch_tiles(kinds):
    """places of the violations inside each tile.  ("gap", g): two violations with exactly g quiet values between them, the
    first 2100 values into the tile (the scan resumes behind it); ("tail", N): a violation 100 values behind another one, so
    that the serial run behind it has N values left to the end of the tile; ("early",): a violation 101 values into the tile,
    its serial run ends inside the tile and the scan resumes at a place that is no multiple of 8"""
    out = []
    for t, kind in enumerate(kinds):
        if kind[0] == "gap":
            at = [2100, 2100 + 1 + kind[1]]
            if kind[1] >= SERIAL_BELOW:
                at.append(at[1] + 1 + 300)
        elif kind[0] == "tail":
            b = TILE - kind[1] - 1
            at = [b - 101, b]
        else:
            at = [101, 101 + 1 + SERIAL_RUN + 2500, 101 + 1 + SERIAL_RUN + 2500 + 51]
        out += [t * TILE + a for a in at]
    return out


def stretches(pad, rng, places):
    """the sum sits in the middle of [1024, 2048) or of [2048, 4096); +-1024 at each of `places` moves it to the other"""
    q = Seq(pad, rng)
    q.add(1536.0)
    for j, p in enumerate(places):
        q.quiet_until(p)
        assert not pad[p]
        q.add(1024.0 if j % 2 == 0 else -1024.0)
    return q.finish(QUIET)


def absorption(pad, rng):
    """1.5 * 2^40 + one ulp (an odd mantissa in the middle of its binade) first; 3000 values below half an ulp; then half-ulps and whole ulps in a mix (a
    half-ulp moves an odd mantissa and not an even one); then its negative, and small values to the end"""
    q = Seq(pad, rng)
    big, u = f32(1.5 * 2.0 ** 40 + 2.0 ** 17), f32(2.0 ** 17)
    q.add(big)
    free = int((~pad[q.i:]).sum())
    small = (np.exp2(rng.uniform(-10, 15.9, 3000)) * rng.choice([-1.0, 1.0], 3000)).astype(np.float32)
    for x in small:
        q.add(x)
    assert q.s == big
    steps = (0.5, -0.5, 1.0, -1.0, 1.5, -1.5, 1.0, -1.0)
    for k in rng.integers(0, len(steps), 3000):
        q.add(f32(steps[k]) * u)
    q.add(-big)
    assert free > 6100 and abs(float(q.s)) < 2.0 ** 30
    while q.i < q.n:
        if q.pad[q.i]:
            q.i += 1
        else:
            q.add(f32(rng.uniform(-4, 4)))
    assert q.v[-1] != 0
    return q.v


def magnitude(pad, rng):
    """the sum near 1.25 (ulp 2^-23): values of exactly 2^26 ulps (8.0), of more, and the largest float below 2^26 ulps"""
    q = Seq(pad, rng)
    q.add(1.25)
    below = f32(8.0 - 4 * 2.0 ** -23)
    for x in (8.0, below, 24.0, 16.0):
        q.quiet(2100)
        assert 1 <= q.s < 2
        q.add(x); q.quiet(3); q.add(-x)
    q.quiet(2100)
    q.add(1.0e30); q.add(-1.0e30)                          # everything absorbed, and back to exactly zero
    assert q.s == 0
    q.add(1.25)
    return q.finish(QUIET)


def tiny(pad, rng, grow):
    """normal floats between 2^-120 and 2^-104, the sign chosen so that the sum stays below 2^-103 (exponent field below 24:
    one addition per step), ending at 2^-106 or more (the centroid is a normal float); grow: the second half climbs to 2^-30"""
    q = Seq(pad, rng)
    free = int((~pad).sum())
    n_tiny = free // 2 if grow else free - 8
    mag = np.exp2(rng.uniform(-120, -104, n_tiny)).astype(np.float32)
    sg = rng.choice([-1.0, 1.0], n_tiny)
    for m, g in zip(mag, sg):
        if abs(float(q.s)) >= 2.0 ** -105:
            g = -np.sign(float(q.s))
        q.add(f32(g) * m)
    rest = free - n_tiny
    if grow:
        ex = np.linspace(-103, -30, rest) + rng.uniform(-1, 1, rest)
        for e, g in zip(ex, rng.choice([-1.0, 1.0, 1.0], rest)):
            q.add(f32(g * 2.0 ** e))
    else:
        for _ in range(rest):
            q.add(f32(2.0 ** -105) if q.s < f32(2.0 ** -105.5) else f32(2.0 ** -112 * rng.uniform(1, 2)))
    assert q.i <= q.n and q.v[-1] != 0
    return q.v


def mixed(pad, rng, mean, sd):
    v = rng.normal(mean, sd, len(pad)).astype(np.float32)
    v[pad] = 0
    assert v[-1] != 0
    return v


def sweep_sequence(pad, rng, lo, hi, share):
    """magnitudes log-uniform over 2^lo .. 2^hi, random signs; a share of the values is (k + 1/2) ulps of the running
    reference sum at that place"""
    q = Seq(pad, rng)
    free = np.nonzero(~pad)[0]
    x = (np.exp2(rng.uniform(lo, hi, len(free))) * rng.choice([-1.0, 1.0], len(free))).astype(np.float32)
    partner = np.nonzero(rng.random(len(free)) < share)[0]
    partner = partner[partner > 0]
    k = rng.integers(-3, 3, len(partner)) + 0.5
    at = 0
    s = f32(0)
    for j, p in enumerate(partner):
        if p > at:
            s = np.add.accumulate(np.concatenate([[s], x[at:p]]).astype(np.float32), dtype=np.float32)[-1]
        if s != 0 and np.isfinite(s):
            x[p] = f32(k[j]) * ulp(s)
        s = f32(s + x[p])
        at = p + 1
    if x[-1] == 0:
        x[-1] = f32(1.0)
    q.v[free] = x
    return q.v


# ---------------------------------------------------------------- clouds


class Case:
    def __init__(self, name, ky, kz, pad, rng, **notes):
        self.name, self.ky, self.kz, self.pad, self.notes = name, ky, kz, pad, notes
        n = len(pad)
        assert len(ky) == len(kz) == n and not pad[-1] and not ky[pad].any() and not kz[pad].any()
        self.finite = int((~pad).sum())
        assert self.finite & (self.finite - 1) == 0       # a power of two: sum / float(count) is exact
        pts = np.empty((n, 3), np.float32)
        pts[:, 0] = np.linspace(0.0, 120.0, n) if n > 1 else 0.0
        pts[:, 1], pts[:, 2] = ky, kz
        junk = (np.exp2(rng.uniform(-10, 30, (n, 3))) * rng.choice([-1.0, 1.0], (n, 3))).astype(np.float32)
        how = rng.integers(0, 6, n)
        for i in np.nonzero(pad)[0]:                      # a padding point: one or all coordinates non-finite, the others anything
            pts[i] = junk[i]
            if how[i] == 5:
                pts[i] = np.nan
            else:
                pts[i, (0, 1, 2, 1, 2)[how[i]]] = (np.nan, np.inf, np.nan, -np.inf, np.inf)[how[i]]
        if "nan_z" in notes:
            i = notes["nan_z"]
            assert pad[i]
            pts[i] = (junk[i, 0], junk[i, 1], np.nan)     # NaN in z only: its x and y are left out too
        self.pts = pts
        self._ref = self._oracle = None

    def reference(self):
        """(centroid, covariance 3x3) from numpy: the plain sequential float sums over the finite points, in index order"""
        if self._ref is None:
            Q = self.pts[np.isfinite(self.pts).all(axis=1)]
            assert len(Q) == self.finite
            with np.errstate(over="ignore", invalid="ignore"):
                sums = np.array([np.add.accumulate(Q[:, d], dtype=np.float32)[-1] for d in range(3)], np.float32)
                c = sums / f32(len(Q))
                D = Q - c
                cov = np.zeros((3, 3), np.float32)
                prods = {}
                for (i, j) in [(1, 1), (1, 2), (2, 2), (0, 0), (0, 1), (0, 2)]:
                    prod = (D[:, j] * D[:, i]).astype(np.float32) if i == 0 else (D[:, i] * D[:, j]).astype(np.float32)
                    prods[i, j] = prod
                    cov[i, j] = cov[j, i] = np.add.accumulate(prod, dtype=np.float32)[-1]
            self._ref = (c, cov, sums, prods)
        return self._ref

    def oracle(self, oracle_mod):
        if self._oracle is None:
            o = oracle_mod.Oracle(self.pts, change_range=0)
            rc, _, c, cov = o.trans2center()
            o.close()
            self._oracle = (rc, c, cov)
        return self._oracle


_cache = {}


def shared(name, make):
    """computed once and shared by the tests that need it (they leave it unchanged)"""
    if name not in _cache:
        _cache[name] = make()
    return _cache[name]


def _families():
    out = []

    def case(name, seed, n, build, reserved=(), finite=None, **notes):
        rng = np.random.default_rng(seed)
        pad = choose_pads(n, rng, reserved, finite)
        ky, kz = build(pad, rng)
        out.append(Case(name, ky, kz, pad, rng, **notes))

    # 1. ties, both parities: positive in y, negative in z; at ulp 1 and with the sum near 2^10 (ulp 2^-13)
    case("ties-ulp1", 101, 9001, lambda p, r: (ties(p, r, 1.0, 1.0), ties(p, r, -1.0, 1.0)))
    case("ties-ulp2^-13", 102, 8400, lambda p, r: (ties(p, r, 1.0, 2.0 ** -13), ties(p, r, -1.0, 2.0 ** -13)))
    # 2. exact landings
    case("landings-2^24", 201, 24577, lambda p, r: (landings_top(p, r, 1.0, 1.0), landings_top(p, r, -1.0, 2.0 ** -5)))
    case("landings-2^23", 202, 24577, lambda p, r: (landings_bottom(p, r, 1.0, 1.0), landings_bottom(p, r, -1.0, 2.0 ** -5)))
    # 3. returns to zero
    case("zero-returns", 301, 6000, lambda p, r: (zero_returns(p, r, False), zero_returns(p, r, True)))
    lead = np.arange(4096, 12288 - 1)                      # the first 4096 points are the padding: the first finite point is late
    case("zero-returns-late-first-point", 302, 12288, lambda p, r: (zero_returns(p, r, False), zero_returns(p, r, True)), reserved=lead)
    # 4. binade churn: longer than 4096, across a tile boundary, ending in the last few values of a tile
    case("churn", 401, 18384, lambda p, r: (churn(p, r, [(3000, 2 * TILE - 4)]), churn(p, r, [(0, TILE - 2), (12000, 18384)])))
    # 5. violation distances and serial-run remainders
    ya, za = stretch_tiles([("gap", 2046), ("tail", 63), ("tail", 127)]), stretch_tiles([("gap", 2047), ("tail", 64), ("tail", 128)])
    yb, zb = stretch_tiles([("gap", 2048), ("tail", 65), ("tail", 129)]), stretch_tiles([("gap", 2049), ("tail", 130), ("early",)])
    case("stretches-a", 501, 3 * TILE + 1, lambda p, r: (stretches(p, r, ya), stretches(p, r, za)), reserved=[0] + ya + za, places=(ya, za))
    case("stretches-b", 502, 3 * TILE + 1, lambda p, r: (stretches(p, r, yb), stretches(p, r, zb)), reserved=[0] + yb + zb, places=(yb, zb))
    # 6. absorption and magnitude
    case("absorption-magnitude", 601, 17500, lambda p, r: (absorption(p, r), magnitude(p, r)))
    # 7. tiny sums: y and z stay tiny to the end (their products underflow to exactly zero); then y grows out of it beside an
    #    ordinary z (a tiny y beside a z of 2^-40 would make denormal products)
    case("tiny", 701, 2500, lambda p, r: (tiny(p, r, False), tiny(p, r, False)))
    case("tiny-grows", 702, 5000, lambda p, r: (tiny(p, r, True), mixed(p, r, 40.0, 100.0)))
    # 8. lengths; a point that is NaN in z only somewhere inside (n = 1 has no inside)
    for n in LENGTHS:
        finite = 1 if n == 1 else 1 << ((n - 1).bit_length() - 1)
        rng = np.random.default_rng(800 + n)
        pad = choose_pads(n, rng, finite=finite)
        notes = dict(nan_z=int(np.nonzero(pad)[0][len(np.nonzero(pad)[0]) // 2])) if n > 1 else {}
        out.append(Case("length-%d" % n, mixed(pad, rng, 0.0, 100.0), mixed(pad, rng, 300.0, 200.0), pad, rng, **notes))
    # 9. overflow: every point finite, the y sum reaches +inf
    case("overflow", 901, 600, lambda p, r: (np.where(p, 0, r.uniform(1e36, 3e36, len(p))).astype(np.float32), mixed(p, r, 5.0, 50.0)))
    return out


def families():
    return shared("families", _families)


def family(name):
    return next(c for c in families() if c.name == name)


FAMILY_NAMES = ["ties-ulp1", "ties-ulp2^-13", "landings-2^24", "landings-2^23", "zero-returns", "zero-returns-late-first-point", "churn",
                "stretches-a", "stretches-b", "absorption-magnitude", "tiny", "tiny-grows"] + ["length-%d" % n for n in LENGTHS] + ["overflow"]


def _sweep():
    """10. about a hundred random sequences; case i is built from default_rng([SWEEP_SEED, i])"""
    out = []
    for i in range(SWEEP_COUNT):
        rng = np.random.default_rng([SWEEP_SEED, i])
        finite = 1 << int(rng.integers(0, 15))
        share = rng.uniform(0, 0.5) if rng.random() < 0.85 else 0.0
        n = int(min(20000, max(finite, np.ceil(finite / (1.0 - share)))))
        pad = choose_pads(n, rng, finite=finite)
        ky, kz = (sweep_sequence(pad, rng, *sorted(rng.uniform(-20, 20, 2)), share=rng.uniform(0, 0.2)) for _ in range(2))
        out.append(Case("sweep-%d" % i, ky, kz, pad, rng))
    return out


def sweep():
    return shared("sweep", _sweep)


# ---------------------------------------------------------------- CPU: the inputs are what they claim to be


def test_family_names_are_complete():
    assert [c.name for c in families()] == FAMILY_NAMES
    assert all(len(c.pts) <= 25000 for c in families() + sweep())


def test_ties_meet_both_parities():
    for name in ("ties-ulp1", "ties-ulp2^-13"):
        c = family(name)
        for v, negative in ((c.ky, False), (c.kz, True)):
            k = census(v)
            print(name, "negative" if negative else "positive", {x: k[x] for x in ("ties_even", "ties_odd", "binade_changes", "negative_steps")})
            assert k["ties_odd"] >= 1000 and k["ties_even"] >= 1000
            assert k["binade_changes"] == 1 and k["viol"].max() == k["first_nonzero"]       # 0 -> the binade, and never out of it
            assert (k["negative_steps"] > 8000) == negative
            assert bits(np.abs(v[v != 0][:1]))[0] & 1 == 1 and abs(float(v[v != 0][0])) == 8388609.0 * (1.0 if name == "ties-ulp1" else 2.0 ** -13)


def test_landings_are_exact():
    c = family("landings-2^24")
    for v, negative in ((c.ky, False), (c.kz, True)):
        k = census(v)
        print("2^24", {x: k[x] for x in ("up", "up_tie", "up_exact", "up_rounded", "negative_steps")}, k["stretches"])
        assert k["up"] == 4 and k["up_tie"] == 2 and k["up_exact"] == 1 and k["up_rounded"] == 1    # (a fifth passes 2^24: 2^24 - 1 + 4)
        assert (k["negative_steps"] > 16000) == negative
        assert (k["stretches"] >= SERIAL_RUN).sum() >= 5           # every landing is met by the scan, not inside a serial run
    c = family("landings-2^23")
    for v, negative in ((c.ky, False), (c.kz, True)):
        k = census(v)
        print("2^23", {x: k[x] for x in ("bottom", "bottom_exact", "bottom_rounded", "below_bottom", "negative_steps")}, k["stretches"])
        assert k["bottom_exact"] >= 1 and k["bottom_rounded"] >= 1
        assert k["below_bottom"] >= 3                               # from above 2^23 onto 2^23 - 1/2: only the finer grid holds it
        assert (k["negative_steps"] > 16000) == negative
        assert (k["stretches"] >= SERIAL_RUN).sum() >= 5
        last = k["viol"][-1]                                        # ... the last of them near the end, nothing coarser behind it
        assert len(v) - last < 500 and float(abs(k["acc"][last])) == 8388607.5 * (1.0 if not negative else 2.0 ** -5)
        assert k["binade_changes"] and k["changes_at"][-1] == last


def test_zero_returns_and_late_starts():
    for name in ("zero-returns", "zero-returns-late-first-point"):
        c = family(name)
        k = census(c.ky)
        print(name, "y", {x: k[x] for x in ("zero_returns", "first_nonzero", "low_e")})
        assert k["zero_returns"] >= 500 and k["first_nonzero"] >= 300
        lead = c.ky[: k["first_nonzero"]][~c.pad[: k["first_nonzero"]]]
        assert np.signbit(lead).sum() >= 100 and (~np.signbit(lead)).sum() >= 100     # +0 and -0
        k = census(c.kz)
        print(name, "z", {x: k[x] for x in ("zero_returns", "first_nonzero", "low_e")})
        assert k["first_nonzero"] >= len(c.kz) - 64 and k["zero_returns"] >= 10
    assert family("zero-returns-late-first-point").pad[:4096].all()


def test_churn_changes_binade_at_almost_every_addition():
    c = family("churn")
    for v, runs in ((c.ky, [(3000, 2 * TILE - 4)]), (c.kz, [(0, TILE - 2), (12000, len(c.kz))])):
        ch = np.zeros(len(v), bool)
        ch[census(v)["changes_at"]] = True
        for a, b in runs:
            live = ~c.pad[a:b]
            print("churn run [%d, %d): %d of %d additions change binade" % (a, b, int(ch[a:b][live].sum()), int(live.sum())))
            assert ch[a:b][live].sum() >= 0.99 * live.sum() - 2
    assert 2 * TILE - 4 - 3000 > SERIAL_RUN and 3000 < TILE < 2 * TILE - 4      # longer than a serial run, across a tile boundary,
    assert (2 * TILE - 4) % TILE >= TILE - 8 and (TILE - 2) % TILE >= TILE - 8   # and ending in the last few values of a tile


def test_stretches_hit_both_sides_of_the_serial_threshold():
    """the violations are where they were put and nowhere else; what follows from that and the kernel's three constants: the
    length of every stretch the scan runs over, where every serial run starts and how many values it has left in its tile"""
    gaps, starts, tails, inside = set(), set(), set(), 0
    for name in ("stretches-a", "stretches-b"):
        c = family(name)
        for v, places in zip((c.ky, c.kz), c.notes["places"]):
            k = census(v)
            assert list(k["viol"]) == [0] + places
            assert set(GAPS) & set(int(x) for x in k["stretches"])
            done = 1                                                  # (the first value is added to zero on its own)
            for b in places:
                if b // TILE > done // TILE or done % TILE == 0:
                    done = (b // TILE) * TILE                         # a new tile starts a new scan
                assert b >= done                                      # no violation is hidden inside a serial run
                gaps.add(b - done)
                if b - done < SERIAL_BELOW:
                    end = min((b // TILE + 1) * TILE, b + 1 + SERIAL_RUN)
                    starts.add((b + 1) & 3)
                    tails.add(end - (b + 1))
                    inside += end % TILE != 0
                    done = end
                else:
                    done = b + 1
    print("stretches", sorted(gaps), "serial runs start at (b + 1) & 3 =", sorted(starts), "with", sorted(tails), "values; ending inside a tile:", inside)
    assert set(GAPS) <= gaps and starts == {0, 1, 2, 3} and set(TAILS) <= tails and inside >= 1
    assert SERIAL_BELOW - 1 in GAPS and SERIAL_BELOW in GAPS


def test_absorption_and_magnitude():
    c = family("absorption-magnitude")
    k = census(c.ky)
    print("absorption", {x: k[x] for x in ("absorbed", "ties_even", "ties_odd", "zero_returns")})
    assert c.ky[~c.pad][0] == f32(1.5 * 2.0 ** 40 + 2.0 ** 17) and k["absorbed"] >= 3000 + 300
    assert k["ties_odd"] >= 300 and k["ties_even"] >= 300            # half an ulp moves the odd mantissa, not the even one
    assert (c.ky == -f32(1.5 * 2.0 ** 40 + 2.0 ** 17)).sum() == 1
    k = census(c.kz)
    print("magnitude", {x: k[x] for x in ("big", "near_big", "zero_returns")})
    assert k["big"] >= 4 and k["near_big"] >= 1 and k["zero_returns"] == 1
    at = np.nonzero(c.kz == f32(8.0))[0][0]
    assert k["acc"][at - 1] >= 1 and k["acc"][at - 1] < 2 and (c.kz == f32(8.0 - 4 * 2.0 ** -23)).sum() == 1    # 2^26 ulps of a sum in [1, 2); 2^26 - 4


def test_tiny_sums_have_no_binade():
    c = family("tiny")
    for v in (c.ky, c.kz):
        k = census(v)
        print("tiny: steps without a binade %d of %d, final sum %r" % (k["low_e"], len(v), k["acc"][-1]))
        assert k["low_e"] == len(v) and 2.0 ** -106 <= k["acc"][-1] < 2.0 ** -103
        a = np.abs(v[v != 0])
        assert a.min() >= 2.0 ** -120 and a.max() <= 2.0 ** -104 and len(a) == c.finite
    c = family("tiny-grows")
    k = census(c.ky)
    print("tiny-grows: steps without a binade %d of %d, final sum %r" % (k["low_e"], len(c.ky), k["acc"][-1]))
    assert k["low_e"] >= 2000 and len(c.ky) - k["low_e"] >= 1000 and abs(k["acc"][-1]) > 2.0 ** -40
    a = np.abs(c.ky[c.ky != 0])
    assert a.min() >= 2.0 ** -120 and (a <= 2.0 ** -104).sum() >= 2000


def test_lengths_and_their_nan_z_points():
    for n in LENGTHS:
        c = family("length-%d" % n)
        assert len(c.pts) == n and c.finite == (1 if n == 1 else 1 << ((n - 1).bit_length() - 1))
        if n > 1:
            i = c.notes["nan_z"]
            p = c.pts[i]
            assert c.pad[i] and i < n - 1 and np.isfinite(p[0]) and np.isfinite(p[1]) and np.isnan(p[2])
        if n > 100:
            assert (c.ky > 0).any() and (c.ky < 0).any() and census(c.ky)["binade_changes"] > 20


def test_overflow_case_is_finite_points_only():
    c = family("overflow")
    Q = c.pts[~c.pad]
    assert np.isfinite(Q).all()
    c0, cov, sums, _ = c.reference()
    assert np.isposinf(sums[1]) and np.isposinf(c0[1]) and np.isfinite(c0[[0, 2]]).all() and not np.isfinite(cov).all()


def test_sweep_is_spread():
    n = np.array([len(c.pts) for c in sweep()])
    share = np.array([c.pad.mean() for c in sweep()])
    odd = sum(census(c.ky)["ties_odd"] + census(c.kz)["ties_odd"] for c in sweep())
    print("sweep: %d cases, n %d .. %d, non-finite share up to %.2f, odd-parity ties %d" % (len(n), n.min(), n.max(), share.max(), odd))
    assert len(n) == SWEEP_COUNT and n.min() <= 4 and n.max() >= 15000 and share.max() > 0.3 and (share == 0).any() and odd >= 1000


def test_divisions_are_exact_and_nothing_is_denormal():
    """sum / float(count) loses nothing (a power of two, a normal quotient): an ulp in a sum is an ulp in the centroid; and no
    value, product or partial sum of any case is a non-zero denormal"""
    tiniest = np.finfo(np.float32).tiny
    for c in families() + sweep():
        cen, cov, sums, prods = c.reference()
        if c.name == "overflow":
            continue
        assert (cen * f32(c.finite)).tobytes() == sums.tobytes(), c.name
        assert ((cen == 0) | (np.abs(cen) >= tiniest)).all(), c.name
        Q = c.pts[~c.pad]
        for v in [Q[:, 0], Q[:, 1], Q[:, 2]] + list(prods.values()):
            a = np.abs(np.concatenate([v, np.add.accumulate(v, dtype=np.float32)]))
            assert ((a == 0) | (a >= tiniest)).all(), c.name


def test_oracle_equals_the_numpy_accumulation(oracle_mod):
    """the oracle's trans2center against np.add.accumulate on every case, bit for bit (its build neither contracts nor reorders)"""
    bad = []
    for c in families() + sweep():
        cen, cov, _, _ = c.reference()
        rc, oc, ocov = c.oracle(oracle_mod)
        if rc not in (0, -2) or not same(oc, cen) or not same(ocov, cov):
            bad.append((c.name, rc))
    assert not bad, bad


# ---------------------------------------------------------------- GPU


def same(got, want):
    """the same bytes; where the expectation is not finite (the overflow case), the same isnan / isinf pattern and the same
    bytes in the finite places: the sign bit of a NaN differs between hosts"""
    got, want = np.ascontiguousarray(got, np.float32).ravel(), np.ascontiguousarray(want, np.float32).ravel()
    if np.isfinite(want).all():
        return got.tobytes() == want.tobytes()
    fin = np.isfinite(want)
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isposinf(got), np.isposinf(want)) and
            np.array_equal(np.isneginf(got), np.isneginf(want)) and got[fin].tobytes() == want[fin].tobytes())


def engine_sums(engine_mod, c):
    """ppp_trans2center on a fresh handle, called directly: centroid3 and covariance9 are written before the eigen-solve and the
    re-plan, so they are there whenever the code is PPP_OK, PPP_ERR_DOMAIN or PPP_ERR_CAPACITY"""
    e = engine_mod.Engine(0, change_range=0, trim=TRIM)
    try:
        e.set_cloud(c.pts)
        T, cen, cov = np.zeros(16, np.float32), np.full(3, 12345.0, np.float32), np.full(9, 12345.0, np.float32)
        rc = e.L.ppp_trans2center(e.h, engine_mod._f(T), engine_mod._f(cen), engine_mod._f(cov))
        msg = e.L.ppp_last_error(e.h).decode() if rc else ""
    finally:
        e.close()
    return rc, msg, cen, cov.reshape(3, 3)


def disagreements(engine_mod, oracle_mod, c):
    """what differs for one case, as a list of words (empty: nothing)"""
    rc, msg, cen, cov = engine_sums(engine_mod, c)
    if rc not in (engine_mod.OK, engine_mod.ERR_DOMAIN, engine_mod.ERR_CAPACITY):
        return ["code %d: %s" % (rc, msg)]
    want_c, want_cov, _, _ = c.reference()
    rc_o, oc, ocov = c.oracle(oracle_mod)
    out = []
    for d in range(3):
        if not same(cen[d], want_c[d]):
            out.append("centroid %s: %r, numpy %r" % ("xyz"[d], cen[d], want_c[d]))
    for (i, j) in [(1, 1), (1, 2), (2, 2), (0, 0), (0, 1), (0, 2)]:
        if not same(cov[i, j], want_cov[i, j]) or not same(cov[j, i], want_cov[j, i]):
            out.append("covariance %s%s: %r, numpy %r" % ("xyz"[i], "xyz"[j], cov[i, j], want_cov[i, j]))
    if not same(cen, oc) or not same(cov, ocov):
        out.append("differs from the oracle")
    allowed = {0: (engine_mod.OK, engine_mod.ERR_CAPACITY), -2: (engine_mod.ERR_DOMAIN,)}.get(rc_o, ())
    if rc not in allowed:                                  # (the oracle has no plan to refuse: PPP_ERR_CAPACITY is its 0)
        out.append("code %d (%s), oracle %d" % (rc, msg, rc_o))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", FAMILY_NAMES)
def test_running_sums_of_a_family(engine_mod, oracle_mod, name):
    """centroid and raw covariance sums against numpy's sequential float32 accumulation and against the oracle: the same bytes
    (overflow: the same non-finite pattern)"""
    bad = disagreements(engine_mod, oracle_mod, family(name))
    assert not bad, (name, bad)


@pytest.mark.gpu
def test_running_sums_of_the_seeded_sweep(engine_mod, oracle_mod):
    """a failing case is reported as default_rng([SWEEP_SEED, index])"""
    bad = []
    for i, c in enumerate(sweep()):
        d = disagreements(engine_mod, oracle_mod, c)
        if d:
            bad.append(("seed [%d, %d]" % (SWEEP_SEED, i), len(c.pts), d))
    assert not bad, (len(bad), bad[:5])
