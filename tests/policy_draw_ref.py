"""Host replicas of the two device draws, from their documented definitions (numpy only).

1. The policy kernel's sampled action (k_policy_act, bg_mlp.hip): Gumbel-max over the
   masked logits, the noise a pure function of (seed, step, row, action):

       mix32(x)   lowbias32:  x ^= x >> 16; x *= 0x7FEB352D; x ^= x >> 15; x *= 0x846CA68B;
                              x ^= x >> 16                                  (mod 2^32)
       K          = mix32(mix32(lo ^ mix32(hi + 0x9E3779B9)) ^ step),  lo / hi = the 32-bit
                    words of seed mod 2^64, step mod 2^32 (the call's step plus its device
                    counter, added mod 2^32)
       row key    = K ^ (row * 0x85EBCA6B mod 2^32),  row = the row's index in the call
       word(a)    = mix32(row key ^ (a * 0xC2B2AE35 mod 2^32))
       u          = ((word >> 9) + 1/2) / 2^23  in (0, 1)
       g          = -log(-log(u))
       action     = argmax over a < n_actions of masked_logit[a] + g[a]

   The words are exact here; everything after them is fp64 (gumbel64 is the true value of
   the formula, not the kernel's fp32 evaluation of it).  Equal keys go to the lower
   action, as in the kernel.

2. The arena's uniformly random opponent (k_random_act, bg_engine.hip):

       mix64(x)   murmur3's finalizer:  x ^= x >> 33; x *= 0xFF51AFD7ED558CCD; x ^= x >> 33;
                                        x *= 0xC4CEB9FE1A85EC53; x ^= x >> 33    (mod 2^64)
       h          = mix64(mix64(seed ^ 0x9E3779B97F4A7C15) + ((step << 32) | lane))
       action     = ((h >> 32) * count) >> 32        (0 when count is 0)

Shared by test_policy_draw_ref_cpu.py (what the hashes themselves must satisfy) and
test_gpu_policy_draw.py (the kernels against these)."""
import numpy as np

M32 = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
MASK_LOG = float(np.float32(-103.27892990343185))     # fp32 log(1e-45): the mask of an illegal action
ROW_MUL, ACT_MUL = 0x85EBCA6B, 0xC2B2AE35


def _u32(x):
    """x mod 2^32 as a uint32 array (Python ints of any size and sign, or integer arrays)."""
    if isinstance(x, (int, np.integer)):
        return np.array(int(x) & M32, np.uint32)
    a = np.asarray(x)
    if a.dtype == np.uint32:
        return a
    return (a.astype(np.int64) & M32).astype(np.uint32)


def mix32(x):
    """lowbias32 on uint32 arrays (a bijection of the 32-bit words)."""
    x = _u32(x)
    shape = x.shape
    x = x.reshape(-1).copy()                           # 1-d: array arithmetic wraps mod 2^32
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7FEB352D)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846CA68B)
    x ^= x >> np.uint32(16)
    return x.reshape(shape)


def row_key(seed, step, rows):
    """The noise key of each row (uint32); step and rows broadcast against each other."""
    seed = int(seed) & M64
    lo, hi = seed & M32, seed >> 32
    k = mix32(mix32(lo ^ int(mix32((hi + 0x9E3779B9) & M32))) ^ _u32(step))
    r = np.atleast_1d(_u32(rows))
    return k ^ (r * np.uint32(ROW_MUL))


def noise_words(seed, step, rows, n_actions):
    """uint32 [len(rows) or len(step), n_actions]: the noise word of every (row, action)."""
    a = np.arange(n_actions, dtype=np.uint32) * np.uint32(ACT_MUL)
    return mix32(row_key(seed, step, rows)[:, None] ^ a[None, :])


def gumbel64(w):
    """-log(-log(u)), u = ((w >> 9) + 1/2) / 2^23, in fp64 (log1p: exact near u = 1)."""
    u = ((_u32(w) >> np.uint32(9)).astype(np.float64) + 0.5) / 8388608.0
    return -np.log(-np.log1p(u - 1.0))


def draw(masked_logits64, seed, step, rows, n_actions=None, chunk=8192):
    """Per row: (the drawn action, the runner-up, key[action] - key[runner-up] >= 0) of
    keys = masked_logits64[:, :n_actions] + gumbel64(words).  Columns at or beyond
    n_actions (the value column, the padding) never take part."""
    z = np.asarray(masked_logits64, np.float64)
    A = z.shape[1] if n_actions is None else int(n_actions)
    n = z.shape[0]
    step, rows = np.atleast_1d(_u32(step)), np.atleast_1d(_u32(rows))
    win, run, gap = np.empty(n, np.int64), np.empty(n, np.int64), np.empty(n, np.float64)
    for i in range(0, n, chunk):
        s = slice(i, min(i + chunk, n))
        keys = z[s, :A] + gumbel64(noise_words(seed, step[s] if len(step) > 1 else step,
                                               rows[s] if len(rows) > 1 else rows, A))
        ar = np.arange(keys.shape[0])
        w = keys.argmax(1)                             # the first of equal keys: the lower action
        kw = keys[ar, w]
        if A > 1:
            keys[ar, w] = -np.inf
            r = keys.argmax(1)
            kr = keys[ar, r]
        else:
            r, kr = w, np.full(len(w), -np.inf)
        win[s], run[s], gap[s] = w, r, kw - kr
    return win, run, gap


def mix64(x):
    """murmur3's 64-bit finalizer on uint64 arrays."""
    x = np.atleast_1d(np.asarray(x, np.uint64)).copy()
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xFF51AFD7ED558CCD)
    x ^= x >> np.uint64(33)
    x *= np.uint64(0xC4CEB9FE1A85EC53)
    x ^= x >> np.uint64(33)
    return x


def random_act(counts, seed, step, lanes=None):
    """int32 per lane: ((h >> 32) * count) >> 32, h hashed from (seed, step, lane); lanes
    default to 0..len(counts)-1; step broadcasts against them (seed mod 2^64, step mod 2^32)."""
    counts = np.atleast_1d(np.asarray(counts)).astype(np.uint64)
    lanes = np.arange(len(counts)) if lanes is None else lanes
    lanes = np.atleast_1d(_u32(lanes)).astype(np.uint64)
    step = np.atleast_1d(_u32(step)).astype(np.uint64)
    s = mix64(np.array([(int(seed) & M64) ^ 0x9E3779B97F4A7C15], np.uint64))
    h = mix64(s + ((step << np.uint64(32)) | lanes))
    return (((h >> np.uint64(32)) * counts) >> np.uint64(32)).astype(np.int32)
