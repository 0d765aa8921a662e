"""Specification of the EMA codebook with random restarts of dead codes (QuantizedBottleneckWithRestarts), in NumPy and
plain Python integers.  The reference wraps an absent third-party package here, so this text -- not that package -- fixes
the behaviour of isi_vq_restart_candidates_f32 / isi_vq_ema_update_restart_f32 ("EMA codebook with random
restarts").  One quantiser: embed [D,K], cluster_size [K], embed_avg [D,K], restart_state = (seed, step, restarts at the
last step, restarts in total)."""
import numpy as np

M64 = (1 << 64) - 1


def mix(x: int) -> int:
    """splitmix64's finaliser, modulo 2^64."""
    x &= M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def row(seed: int, step: int, k: int, N: int) -> int:
    """The row of this rank's [N, D] batch shard that code k is redrawn from at `step`."""
    return mix((mix((seed & M64) ^ mix(step)) + k) & M64) % N


def candidates(z: np.ndarray, seed: int, step: int, K: int, rank: int = 0, world: int = 1):
    """(cand [K,D] float32, cand_bad [K] float32) of one rank: its own codes (k mod world == rank) copy their row of the
    local shard z [N,D]; a row with a non-finite component is written as zeros and flagged; other codes are zero."""
    N, D = z.shape
    cand = np.zeros((K, D), dtype=np.float32)
    bad = np.zeros(K, dtype=np.float32)
    for k in range(K):
        if k % world != rank:
            continue
        v = z[row(seed, step, k, N)]
        if np.all(np.isfinite(v)):
            cand[k] = v
        else:
            bad[k] = 1.0
    return cand, bad


def update(embed, cluster_size, embed_avg, counts, embed_sum, cand, cand_bad, state, decay, eps, threshold, initialize,
           dtype=np.float64):
    """One update from the (summed) statistics.  Returns (embed, cluster_size, embed_avg, dead [K] bool, new state).
    `dtype` float64: the value the fp32 kernel is held to; restarted codes are exact in either."""
    f = dtype
    D, K = embed.shape
    seed, step, _, total = (int(v) for v in state)
    decay_, thr = f(np.float32(decay)), f(np.float32(threshold))
    eps_ = f(np.float32(eps))
    cs = cluster_size.astype(f) * decay_ + (f(1) - decay_) * counts.astype(f)
    ea = embed_avg.astype(f) * decay_ + (f(1) - decay_) * embed_sum.astype(f)
    # the dead test is the fp32 kernel's: taken on the fp32 value of the updated cluster size
    cs32 = (cluster_size.astype(np.float32) * np.float32(decay)
            + (np.float32(1) - np.float32(decay)) * counts.astype(np.float32)).astype(np.float32)
    dead = ((cs32 < np.float32(threshold)) | bool(initialize and step == 0)) & (np.asarray(cand_bad) == 0)
    cs[dead] = thr
    ea[:, dead] = (np.float32(threshold) * cand.astype(np.float32)[dead]).astype(np.float32).T.astype(f)
    n = cs.sum()
    new = ea / ((cs + eps_) / (n + f(K) * eps_) * n)[None, :]
    new[:, dead] = cand.astype(f)[dead].T
    n_dead = int(dead.sum())
    return new, cs, ea, dead, (seed, step + 1, n_dead, total + n_dead)
