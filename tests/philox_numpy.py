"""Host restatement of the library's seeded random draws, for tests: Philox4x32-10 (Salmon et al., "Parallel random numbers: as
easy as 1, 2, 3", SC'11) in vectorised numpy on uint64 masked to 32 bits, the stream table of DESIGN.md ("Random streams"), the
keyed Feistel shuffle and the pixel picks of the epoch ray kernel, and the Box-Muller pairs of the sigma noise.  Written from
the published algorithm and the kernels' comments; it never calls the library.

Every consumer calls philox4x32(counter lo, counter hi, STREAM, 0, seed lo, seed hi): the stream word sits in the third counter
word, so two consumers keyed by one seed never share a block.  Seed 0 means "deterministic" to the samplers and is never a key."""
import numpy as np

U64 = np.uint64
M32 = U64(0xFFFFFFFF)

# consumer -> third counter word (ASCII tags, except the epoch picks)
COAR = 0x636F6172      # 'coar'  sample_coarse jitter            counter i = r*S + s (lo, hi)     word 0
FGDP = 0x66676470      # 'fgdp'  pp_fg_depths jitter             counter i = r*S + s              word 0
PRTB = 0x70727462      # 'prtb'  pp_perturb_samples jitter       counter i = r*S + s              word 0
PDFS = 0x70646673      # 'pdfs'  inverse-CDF u of the samplers   counter r*Ni + i                 word 0
NOIS = 0x6E6F6973      # 'nois'  sigma noise (Box-Muller)        counter = float4 index e // 4    words 0..3
OCCG = 0x6F636367      # 'occg'  occupancy cell points           counter = cell                   words 0..2
EPIX = 0x51ED270B      #         epoch pixel picks               counter = source index i         words 0,1 | 2,3

PHILOX_M0, PHILOX_M1 = U64(0xD2511F53), U64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = U64(0x9E3779B9), U64(0xBB67AE85)


def _u64(x):
    return np.asarray(x).astype(U64) & M32


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Ten rounds on broadcastable arrays of 32-bit values -> four uint32 arrays."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*[_u64(x) for x in (c0, c1, c2, c3, k0, k1)])
    for _ in range(10):
        p0 = PHILOX_M0 * c0                      # < 2^64: both factors < 2^32
        p1 = PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0 = (k0 + PHILOX_W0) & M32
        k1 = (k1 + PHILOX_W1) & M32
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def key(seed):
    seed = int(seed)
    assert 0 <= seed < 2 ** 64
    return seed & 0xFFFFFFFF, seed >> 32


def stream_words(stream, counter, seed):
    """The four words of block `counter` (any integer array below 2^64) of a stream under `seed`."""
    c = np.asarray(counter).astype(U64)
    k0, k1 = key(seed)
    return philox4x32(c & M32, c >> U64(32), stream, 0, k0, k1)


def u01(x):
    """U[0, 1) from the top 24 bits: float32(x >> 8) * 2^-24, exact in fp32."""
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def stream_u(stream, shape, seed):
    """float32 `shape` of u01(word 0) with the flat C-order index as counter: the jitter of coar / fgdp / prtb ([n, S]) and the
    inverse-CDF positions of pdfs ([n, Ni])."""
    n = int(np.prod(shape))
    return u01(stream_words(stream, np.arange(n, dtype=U64), seed)[0]).reshape(shape)


def box_muller(words, std):
    """float64 [..., 4] from the four uint32 arrays of a block, as gauss_noise_kernel pairs them: (w0, w1) -> slots 0, 1 and
    (w2, w3) -> slots 2, 3 with u1 = ((w >> 8) + 0.5) * 2^-24 in (0, 1), u2 = (w >> 8) * 2^-24, r = sqrt(-2 ln u1) * std,
    slots (r cos 2 pi u2, r sin 2 pi u2)."""
    w = [(np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float64) for x in words]
    out = []
    for h in range(2):
        u1 = (w[2 * h] + 0.5) * 2.0 ** -24
        u2 = w[2 * h + 1] * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1)) * float(std)
        out += [r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)]
    return np.stack(out, -1)


def gauss_noise(count, std, seed):
    """float64 [count]: element e of the flat noise buffer = slot e % 4 of block e // 4 of the nois stream."""
    n4 = (int(count) + 3) // 4
    return box_muller(stream_words(NOIS, np.arange(n4, dtype=U64), seed), std).reshape(-1)[:count]


def mix32(x):
    """murmur3's 32-bit finaliser."""
    x = _u64(x)
    x ^= x >> U64(16)
    x = (x * U64(0x85EBCA6B)) & M32
    x ^= x >> U64(13)
    x = (x * U64(0xC2B2AE35)) & M32
    x ^= x >> U64(16)
    return x


def half_bits_of(N):
    """Half the width of the Feistel domain: 2^bits is the first power of two >= N with bits >= 2, rounded up to an even width."""
    bits = 2
    while bits < 62 and (1 << bits) < int(N):
        bits += 1
    return (bits + 1) // 2


def feistel_perm(j, N, k0, k1):
    """Keyed bijection of [0, N): six Feistel rounds on 2 * half_bits bits (round keys k0, k1 alternating, round constant
    0x9E3779B9 * (round + 1), round function mix32 masked to the half), cycle-walked until the value is below N."""
    N = int(N)
    hb = half_bits_of(N)
    assert hb <= 32
    mask = U64((1 << hb) - 1)
    sh = U64(hb)
    x = np.array(j, dtype=U64, ndmin=1, copy=True)
    out = np.empty_like(x)
    todo = np.arange(x.size)
    while todo.size:
        l, r = (x >> sh) & mask, x & mask
        for rnd in range(6):
            rk = U64((k1 if rnd & 1 else k0) & 0xFFFFFFFF)
            rc = U64((0x9E3779B9 * (rnd + 1)) & 0xFFFFFFFF)
            l, r = r, l ^ (mix32(r ^ rk ^ rc) & mask)
        x = (l << sh) | r
        done = x < U64(N)
        out[todo[done]] = x[done]
        todo, x = todo[~done], x[~done]
    return out.astype(np.int64).reshape(np.shape(j))


def epoch_rows(plan, offs, N, seed, shuffle, H, W, weighted=None):
    """The epoch ray kernel's chain for the output rows 0 .. N-1 -> (src int64 [N], leaf_row int64 [N], pix int64 [N, 3]):
    row j <- source index i = feistel_perm(j) (i = j without the shuffle) -> plan row l = the last one with offs[l] <= i ->
    pixel from block i of the epoch-pick stream.  plan: int [L, 7] (image, leaf, count, row_lo, row_hi, col_lo, col_hi); offs: the
    exclusive prefix sums of the counts ([L + 1]).  Uniform pick: lo + ((word * (hi - lo)) >> 32) on words 0 (row) and 1 (column).
    weighted = dict(n_weighted [L], seg_beg [L], seg_end [L], order, cum float64): a source whose index inside its leaf is below
    n_weighted[l] takes pixel order[p], p the first position of the leaf's segment [seg_beg, seg_end) with
    cum[p] > before + u * tot (the segment's last position if there is none), u = ((w2 << 21) ^ (w3 >> 11)) * 2^-53 in float64."""
    plan = np.asarray(plan).astype(np.int64)
    offs = np.asarray(offs).astype(np.int64)
    N = int(N)
    k0, k1 = key(seed)
    rows = np.arange(N, dtype=np.int64)
    src = feistel_perm(rows, N, k0, k1) if (shuffle and N > 0) else rows
    L = plan.shape[0]
    leaf_row = np.searchsorted(offs[:L], src, side='right') - 1
    w = [x.astype(U64) for x in stream_words(EPIX, src, seed)]
    pl = plan[leaf_row]
    row = pl[:, 3] + ((w[0] * (pl[:, 4] - pl[:, 3]).astype(U64)) >> U64(32)).astype(np.int64)
    col = pl[:, 5] + ((w[1] * (pl[:, 6] - pl[:, 5]).astype(U64)) >> U64(32)).astype(np.int64)
    if weighted is not None:
        nw = np.asarray(weighted['n_weighted']).astype(np.int64)
        beg, end = (np.asarray(weighted[k]).astype(np.int64) for k in ('seg_beg', 'seg_end'))
        order = np.asarray(weighted['order']).astype(np.int64)
        cum = np.asarray(weighted['cum'], dtype=np.float64)
        sel = np.nonzero((src - offs[leaf_row]) < nw[leaf_row])[0]
        b, e = beg[leaf_row[sel]], end[leaf_row[sel]]
        before = np.where(b > 0, cum[np.maximum(b - 1, 0)], 0.0)
        tot = cum[e - 1] - before
        u = ((w[2][sel] << U64(21)) ^ (w[3][sel] >> U64(11))).astype(np.float64) * 2.0 ** -53
        target = before + u * tot                      # two roundings: product, then sum
        pos = np.empty(sel.size, dtype=np.int64)
        for q in range(sel.size):                      # per-segment search (the cumulative weights need not be strictly increasing)
            pos[q] = min(b[q] + np.searchsorted(cum[b[q]:e[q]], target[q], side='right'), e[q] - 1)
        flat = order[pos]
        row[sel] = (flat // W) % H
        col[sel] = flat % W
    return src, leaf_row, np.stack([pl[:, 0], row, col], 1)
