"""fp32 numpy restatement of marched training (include/fastnerf.h, "marched training": fastnerf_occ_march_jitter, fastnerf_march_mask), on
top of tests/march_numpy.py and tests/philox_numpy.py: the test oracle of the jittered lattice of csrc/march.hip.

The walk itself is march_numpy.march_round: the kernel is one template, and the shifted instantiation differs from the unshifted one only
in the depths it looks up and stores.  So the restatement is the shifted lattice, the live bits AT the shifted depths, and the same walk."""
import numpy as np

import march_numpy as M
import philox_numpy as P

F32 = np.float32
MRCH = 0x6D726368      # 'mrch'  per-ray lattice shift           counter = r                      word 0


def draw_u(n, seed):
    """float32 [n]: u_r = u01(word 0) of Philox block r of the 'mrch' stream keyed by seed (seed != 0)."""
    assert int(seed) != 0, 'seed 0 means "no shift" and is never a key'
    return P.u01(P.stream_words(MRCH, np.arange(int(n), dtype=P.U64), seed)[0])


def jittered_lattice(rays11, K, u, lindisp=False):
    """float32 [n, K + 1]: z_k(u) = z_k + u_r * (z_{k+1} - z_k) for k < K, and z_K(u) = z_{K-1}(u) + (z_K - z_{K-1}), every operation
    rounded to fp32; z_k = march_numpy.lattice (z_K its closing depth)."""
    z = M.lattice(rays11, K, lindisp)
    u = np.asarray(u, F32).reshape(-1, 1)
    assert u.shape[0] == z.shape[0]
    with np.errstate(all='ignore'):
        w = (z[:, 1:] - z[:, :-1]).astype(F32)                    # fsub(z_{k+1}, z_k), k = 0 .. K-1
        zu = (z[:, :K] + (u * w).astype(F32)).astype(F32)         # fadd(z_k, fmul(u, .))
        zK = (zu[:, K - 1] + w[:, K - 1]).astype(F32)             # fadd(z_{K-1}(u), fsub(z_K, z_{K-1}))
    return np.concatenate([zu, zK[:, None]], -1).astype(F32)


def march(grid, rays11, K, C, u, lindisp=False, B=None):
    """The rows of fastnerf_occ_march_jitter: (z [n, C], kidx [n, C], overflow uint8 [n], state int32 [n, 2]) after the last round
    (segments of B slots; None: one round), and the live bits [n, K] at the shifted depths."""
    zu = jittered_lattice(rays11, K, u, lindisp)
    live = M.live_bits(grid, rays11, zu[:, :K])
    return M.march(live, zu, C, B), live


def mask(overflow, g_rgb):
    """fastnerf_march_mask: a copy of g_rgb [n, 3] with the rows of the overflowed rays zeroed."""
    out = np.array(g_rgb, F32)
    out[np.asarray(overflow) != 0] = 0
    return out
