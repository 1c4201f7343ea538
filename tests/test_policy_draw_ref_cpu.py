"""What the host replica of the device draws (policy_draw_ref.py) must itself satisfy: the
hash design is judged once, here, so that test_gpu_policy_draw.py can compare the kernels
with the replica exactly and on small shapes.

Chi-square limits are the project's rule chi2 < dof + 6 sqrt(2 dof) + 10 over the bins with
p N > 20 (test_gpu_policy.test_policy_sampling_distribution).  The measured values are in
the docstrings; a condition that fails is a finding about the sampler."""
import numpy as np
import pytest

import policy_draw_ref as R

SEEDS_STEPS = [(1, 0), (0xDEADBEEF12, 900), (2 ** 64 - 1, 2 ** 32 - 1)]
ROWS, A = 65_536, 500
N = 200_000
COUNTS = (2, 5, 33, 64, 65, 500, 0)
FIXED_ROW, FIXED_STEP, SEED = 1234, 77, 0xC0FFEE


def _limit(dof):
    return dof + 6 * np.sqrt(2 * dof) + 10


def _chi2(obs, p, n):
    """(chi2, dof) of the counts `obs` against the probabilities p over the bins with p n > 20."""
    keep = p * n > 20
    chi2 = float(((obs[keep] - p[keep] * n) ** 2 / (p[keep] * n)).sum())
    return chi2, int(keep.sum()) - 1


# ---------------------------------------------------------------------- fixed vectors --

def test_mix32_and_words_fixed_values():
    """lowbias32 and murmur3's finalizer on hand-computed words: 0 is a fixed point of both,
    both are bijections (a full 2^16-word slice has no repeated image), and the scalar,
    Python-int path of row_key equals the array path (seed and step taken mod 2^64 / 2^32,
    a negative seed included)."""
    assert int(R.mix32(0)) == 0 and int(R.mix64(0)[0]) == 0
    x = 1                                              # lowbias32(1) step by step in Python ints
    x ^= x >> 16; x = x * 0x7FEB352D & R.M32; x ^= x >> 15; x = x * 0x846CA68B & R.M32; x ^= x >> 16
    assert int(R.mix32(1)) == x
    y = 1
    y ^= y >> 33; y = y * 0xFF51AFD7ED558CCD & R.M64; y ^= y >> 33; y = y * 0xC4CEB9FE1A85EC53 & R.M64; y ^= y >> 33
    assert int(R.mix64(1)[0]) == y
    w = R.mix32(np.arange(1 << 16, dtype=np.uint32) * np.uint32(0x10001))
    assert len(np.unique(w)) == 1 << 16
    rows = np.arange(50)
    for seed, step in ((-1, -1), (-5, 3), (2 ** 64 + 7, 2 ** 32 + 9)):
        a = R.row_key(seed, step, rows)
        b = R.row_key(seed % 2 ** 64, step % 2 ** 32, rows)
        assert a.dtype == np.uint32 and np.array_equal(a, b)
    # seed_hi, seed_lo, the step and the row each move the key
    base = R.row_key(5, 9, rows)
    for other in (R.row_key(5 + (1 << 32), 9, rows), R.row_key(6, 9, rows), R.row_key(5, 10, rows),
                  R.row_key(5, 9, rows + 1)):
        assert not (base == other).any()
    # a step array at one row == the scalar calls
    ks = R.row_key(5, np.arange(4), 17)
    assert [int(k) for k in ks] == [int(R.row_key(5, t, 17)[0]) for t in range(4)]


def test_gumbel64_values():
    """u = ((w >> 9) + 1/2) 2^-23 and -log(-log(u)) at the ends and in the middle: the
    smallest word gives -log(24 log 2) = -2.8117, the largest -log(2^-24 (1 + 2^-25)) =
    16.6355, and the low 9 bits of the word do not enter."""
    g = R.gumbel64(np.array([0, 0x1FF, 0x80000000, 0xFFFFFFFF, 0xFFFFFE00], np.uint32))
    assert g[0] == g[1] and g[3] == g[4]
    assert abs(g[0] + np.log(24 * np.log(2))) < 1e-12
    assert abs(g[2] + np.log(-np.log(0.5 + 2.0 ** -24))) < 1e-12
    v = 2.0 ** -24
    assert abs(g[3] + np.log(v + v * v / 2 + v ** 3 / 3)) < 1e-12
    assert 16.63 < g[3] < 16.64                        # below the kernel's kGumbelMax = 17


def test_draw_ignores_columns_past_n_actions():
    """draw(): columns at or beyond n_actions never win, the winner is the argmax of the keys,
    the gap is key[winner] - key[runner-up], and neither chunking nor slicing the batch
    changes a row's result."""
    rng = np.random.default_rng(0)
    z = rng.normal(0, 2, (300, 40))
    z[:, 33:] = 1e6
    rows = np.arange(300)
    w, r, gap = R.draw(z, 9, 4, rows, n_actions=33)
    assert w.max() < 33 and r.max() < 33 and (gap >= 0).all() and (w != r).all()
    keys = z[:, :33] + R.gumbel64(R.noise_words(9, 4, rows, 33))
    assert np.array_equal(w, keys.argmax(1))
    srt = np.sort(keys, 1)
    assert np.array_equal(gap, srt[:, -1] - srt[:, -2])
    w2, r2, gap2 = R.draw(z, 9, 4, rows, n_actions=33, chunk=7)
    assert np.array_equal(w, w2) and np.array_equal(r, r2) and np.array_equal(gap, gap2)
    # rows [5, 6, 7] of a longer batch draw what a batch of their own with those row ids draws
    w3, _, _ = R.draw(z[5:8], 9, 4, rows[5:8], n_actions=33)
    assert np.array_equal(w3, w[5:8])
    # one action: it wins by an infinite gap
    w1, r1, g1 = R.draw(z[:, :1], 9, 4, rows)
    assert not w1.any() and not r1.any() and np.isposinf(g1).all()


# ------------------------------------------------------------------ the noise words --

@pytest.fixture(scope="module")
def words():
    """uint32 [65,536, 500] per (seed, step) of SEEDS_STEPS, computed once."""
    cache = {}

    def get(seed, step):
        if (seed, step) not in cache:
            cache.clear()                              # 131 MB each: one at a time
            cache[(seed, step)] = R.noise_words(seed, step, np.arange(ROWS), A)
        return cache[(seed, step)]
    return get


@pytest.mark.parametrize("seed,step", SEEDS_STEPS)
def test_u_uniform(words, seed, step):
    """256 bins of the word's top 8 bits (the top of u) and of its bits 9-16 (the bottom of
    u's 23 bits) over 65,536 rows x 500 actions.  Measured chi2 at 255 degrees of freedom:
    219-278."""
    w = words(seed, step)
    n = w.size
    for shift in (24, 9):
        obs = np.bincount(((w >> np.uint32(shift)) & np.uint32(0xFF)).ravel(), minlength=256)
        chi2, dof = _chi2(obs.astype(np.float64), np.full(256, 1 / 256), n)
        print(f"[draw-ref] u bits {shift}-{shift + 7} seed={seed:#x} step={step}: chi2 {chi2:.1f} / {dof}")
        assert dof == 255 and chi2 < _limit(dof), (shift, chi2)


@pytest.mark.parametrize("seed,step", SEEDS_STEPS)
def test_shared_noise_words(words, seed, step):
    """Equal noise words among 65,536 rows x 500 actions.  word = mix32(K ^ row c1 ^ a c2)
    with mix32 a bijection, so two (row, action) pairs share a word exactly where
    row c1 ^ a c2 agree: the pattern does not depend on seed or step.  Measured, as upper
    bounds: no two actions of one row share a word (c2 is odd); 119,982 words repeat an earlier
    one (119,398 words occur twice and 292 three times: 120,274 equal pairs; random words
    would give 125,000); no word occurs more than 3 times; no two rows share more than 6 of
    their 500 words."""
    w = words(seed, step)
    # sort (word, position) as one 64-bit key: the runs of equal words with their rows
    key = (w.ravel().astype(np.uint64) << np.uint64(32)) | np.arange(w.size, dtype=np.uint64)
    key.sort()
    s = (key >> np.uint64(32)).astype(np.uint32)
    row = ((key & np.uint64(R.M32)) // np.uint64(A)).astype(np.int64)
    del key
    start = np.nonzero(np.concatenate([[True], s[1:] != s[:-1]]))[0]
    length = np.diff(np.concatenate([start, [len(s)]]))
    repeats = len(s) - len(start)                      # words beyond their first occurrence
    pairs = int((length * (length - 1) // 2).sum())
    print(f"[draw-ref] shared words seed={seed:#x} step={step}: {repeats} repeated words, {pairs} equal pairs, "
          f"multiplicities {np.bincount(length)[1:].tolist()}")
    assert repeats <= 119_982 and pairs <= 120_274
    assert int(length.max()) <= 3
    # the row pairs behind every equal pair
    ra, rb = [], []
    for d in (1, 2):                                   # runs are at most 3 long
        same = s[d:] == s[:-d]
        ra.append(row[:-d][same])
        rb.append(row[d:][same])
    ra, rb = np.concatenate(ra), np.concatenate(rb)
    assert len(ra) == pairs
    assert int((ra == rb).sum()) == 0                  # within one row: none
    lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
    _, shared = np.unique(lo * ROWS + hi, return_counts=True)
    print(f"[draw-ref] shared words seed={seed:#x} step={step}: two rows share at most {int(shared.max())}")
    assert int(shared.max()) <= 6


# ------------------------------------------------------------- Gumbel-max frequencies --

def _logits():
    """Normal, sd 2.  Seed 0 is the first whose five leading actions all keep more than 1 %
    of the mass at count 5, so every cell of the lag-1 table expects more than 20 draws."""
    return np.random.default_rng(0).normal(0.0, 2.0, A)


def _masked(z, count):
    return np.where(np.arange(A) < count, z, z + R.MASK_LOG)


@pytest.fixture(scope="module", params=["rows", "steps"])
def draws(request):
    """(way, {count: int64[N] drawn actions}) for the fixed logit vector: over rows 0..N-1 at
    one step, or over steps 0..N-1 at one row.  The noise does not depend on the count, so
    each chunk of it serves all seven."""
    way = request.param
    z = _logits()
    masked = np.stack([_masked(z, c) for c in COUNTS])
    out = {c: np.empty(N, np.int64) for c in COUNTS}
    for i in range(0, N, 20_000):
        idx = np.arange(i, min(i + 20_000, N))
        if way == "rows":
            g = R.gumbel64(R.noise_words(SEED, FIXED_STEP, idx, A))
        else:
            g = R.gumbel64(R.noise_words(SEED, idx, FIXED_ROW, A))
        for k, c in enumerate(COUNTS):
            out[c][idx] = (g + masked[k]).argmax(1)
    return way, out


@pytest.mark.parametrize("count", COUNTS)
def test_gumbel_max_frequencies(draws, count):
    """200,000 draws of one logit vector (normal, sd 2, 500 actions; illegal actions carry
    MASK_LOG, count 0 masks all of them) against softmax(masked): over rows at one step, and
    over steps at one row (what a lane sees in self-play).  The first is the reference draw()
    itself.  Measured chi2 / dof: between 0.5 / 1 (count 2 over steps) and 355.0 / 349 (counts
    500 and 0 over steps), the largest excess 84.4 / 62 (count 64 over steps; limit 138.8)."""
    z = _logits()
    m = _masked(z, count)
    way, a = draws[0], draws[1][count]
    if way == "rows":                                  # draw() is the same function
        w, _, _ = R.draw(np.broadcast_to(m, (1000, A)), SEED, FIXED_STEP, np.arange(1000))
        assert np.array_equal(w, a[:1000])
    else:
        w, _, _ = R.draw(np.broadcast_to(m, (1000, A)), SEED, np.arange(1000), FIXED_ROW)
        assert np.array_equal(w, a[:1000])
    p = np.exp(m - m.max())
    p /= p.sum()
    if count:
        assert a.max() < count                         # exp(-103) of mass elsewhere
    chi2, dof = _chi2(np.bincount(a, minlength=A).astype(np.float64), p, N)
    print(f"[draw-ref] frequencies over {way} count={count}: chi2 {chi2:.1f} / {dof}")
    assert dof >= 1 and chi2 < _limit(dof), (way, count, chi2, dof)


def test_lag1_independence(draws):
    """The action at row i against row i + 1, and at step t against step t + 1, with 5 legal
    actions: a 5 x 5 contingency chi-square (16 degrees of freedom) against the product of
    the margins.  Measured: 20.6 over rows and 9.5 over steps (limit 59.9)."""
    way, a = draws[0], draws[1][5]
    tab = np.zeros((5, 5))
    np.add.at(tab, (a[:-1], a[1:]), 1)
    n = tab.sum()
    exp = tab.sum(1)[:, None] * tab.sum(0)[None, :] / n
    assert (exp > 20).all()
    chi2 = float(((tab - exp) ** 2 / exp).sum())
    print(f"[draw-ref] lag-1 over {way}: chi2 {chi2:.1f} / 16")
    assert chi2 < _limit(16), (way, chi2)


# ------------------------------------------------------------------------ random_act --

def test_random_act_range():
    """In [0, count) for count 1, 2, 3, 500 and 65535 (both ends reached where 200,000
    draws can reach them) and 0 for count 0, over lanes and over steps."""
    lanes = np.arange(N)
    for count in (1, 2, 3, 500, 65535):
        for a in (R.random_act(np.full(N, count), 17, 3), R.random_act(np.full(N, count), 17, lanes, lanes=np.full(N, 9))):
            assert a.dtype == np.int32 and a.min() >= 0 and a.max() < count
            if count <= 500:
                assert a.min() == 0 and a.max() == count - 1
    assert not R.random_act(np.zeros(N, np.int64), 17, 3).any()
    # seed mod 2^64, step mod 2^32; every input moves the draw
    c = np.full(1000, 65535)
    assert np.array_equal(R.random_act(c, -1, -1), R.random_act(c, 2 ** 64 - 1, 2 ** 32 - 1))
    base = R.random_act(c, 5, 9)
    for other in (R.random_act(c, 5 + (1 << 32), 9), R.random_act(c, 6, 9), R.random_act(c, 5, 10),
                  R.random_act(c, 5, 9, lanes=np.arange(1, 1001))):
        assert (base != other).mean() > 0.99


@pytest.mark.parametrize("count", [7, 500])
@pytest.mark.parametrize("way", ["lanes", "steps"])
def test_random_act_uniform(way, count):
    """Chi-square uniformity of 200,000 draws over lanes at one step and over steps at one
    lane, count 7 and count 500."""
    c = np.full(N, count)
    if way == "lanes":
        a = R.random_act(c, 0xABCDEF0123, 5)
    else:
        a = R.random_act(c, 0xABCDEF0123, np.arange(N), lanes=np.full(N, 321))
    chi2, dof = _chi2(np.bincount(a, minlength=count).astype(np.float64), np.full(count, 1 / count), N)
    print(f"[draw-ref] random_act over {way} count={count}: chi2 {chi2:.1f} / {dof}")
    assert dof == count - 1 and chi2 < _limit(dof), (way, count, chi2)
