"""The host restatement of the seeded draws (tests/philox_numpy.py) against published known answers and its own invariants, and the
host-side row count of a rank's epoch shard against parallel.shard_global_rows.  No GPU: tests/test_gpu_seeded_draws.py then holds
the kernels to this restatement bit for bit."""
import numpy as np
import pytest

import philox_numpy as P


# Random123's known-answer vectors of philox4x32 with 10 rounds (kat_vectors): counter, key -> output
KAT = [((0x00000000,) * 4, (0x00000000,) * 2, (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize('kat', range(len(KAT)))
def test_philox_known_answers(kat):
    ctr, k, want = KAT[kat]
    got = P.philox4x32(*ctr, *k)
    assert all(g.dtype == np.uint32 for g in got)
    assert tuple(int(g) for g in got) == want


def test_philox_is_vectorised_per_element():
    ctr = np.array([c for c, _, _ in KAT], dtype=np.uint64)
    k = np.array([k for _, k, _ in KAT], dtype=np.uint64)
    got = np.stack(P.philox4x32(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], k[:, 0], k[:, 1]), 1)
    assert np.array_equal(got, np.array([w for _, _, w in KAT], dtype=np.uint32))
    # stream_words splits a 64-bit counter and a 64-bit seed into (lo, hi)
    c, seed = 0x85A308D3243F6A88, 0x299F31D0A4093822
    a = P.stream_words(0x13198A2E, np.array([c], dtype=np.uint64), seed)
    b = P.philox4x32(c & 0xFFFFFFFF, c >> 32, 0x13198A2E, 0, seed & 0xFFFFFFFF, seed >> 32)
    assert [int(x[0]) for x in a] == [int(x) for x in b]
    assert P.key(2 ** 32) == (0, 1) and P.key(2 ** 62 - 1) == (0xFFFFFFFF, 0x3FFFFFFF)


def test_stream_words_are_the_tags_the_kernels_name():
    for tag, word in (('coar', P.COAR), ('fgdp', P.FGDP), ('prtb', P.PRTB), ('pdfs', P.PDFS), ('nois', P.NOIS), ('occg', P.OCCG)):
        assert int.from_bytes(tag.encode(), 'big') == word
    assert P.EPIX == 0x51ED270B
    assert len({P.COAR, P.FGDP, P.PRTB, P.PDFS, P.NOIS, P.OCCG, P.EPIX}) == 7


def test_stream_table_of_the_design_document_and_the_kernels():
    """DESIGN.md's "Random streams" table, the helper and the kernel sources name the same stream words."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, 'DESIGN.md')) as f:
        doc = f.read()
    table = doc[doc.index('### Random streams'):doc.index('## 6. Multi-GPU')]
    rows = [r.split('|') for r in table.splitlines() if r.startswith('|')][2:]          # (header and rule skipped)
    words = [int(re.search(r'`(0x[0-9a-fA-F]{8})`', r[2]).group(1), 16) for r in rows]
    assert words == [P.COAR, P.FGDP, P.PRTB, P.PDFS, P.NOIS, P.OCCG, P.EPIX]
    assert 'Seed 0 means "deterministic"' in table
    csrc = os.path.join(root, 'fast-learning-nerf_amd', 'csrc')
    where = {P.COAR: 'rays.hip', P.FGDP: 'rays.hip', P.PRTB: 'rays.hip', P.EPIX: 'rays.hip', P.PDFS: 'composite.hip', P.NOIS: 'train.hip',
             P.OCCG: 'occupancy.hip'}
    for w, name in where.items():
        with open(os.path.join(csrc, name)) as f:
            assert re.search(r'philox4x32\([^;]*0x%08xu' % w, f.read(), re.I), (hex(w), name)


KEYS = [(0x12345678, 0x9ABCDEF0), (0, 0)]


@pytest.mark.parametrize('N', [1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 257, 1000, 4097])
def test_feistel_perm_is_a_bijection(N):
    for k0, k1 in KEYS:
        p = P.feistel_perm(np.arange(N), N, k0, k1)
        assert p.shape == (N,) and np.array_equal(np.sort(p), np.arange(N)), (N, k0, k1)


def test_feistel_perm_depends_on_both_keys():
    a = P.feistel_perm(np.arange(1000), 1000, 0x12345678, 0x9ABCDEF0)
    assert not np.array_equal(a, P.feistel_perm(np.arange(1000), 1000, 0, 0))
    assert not np.array_equal(a, P.feistel_perm(np.arange(1000), 1000, 0x12345678, 0x12345678))      # k1 matters
    assert not np.array_equal(a, P.feistel_perm(np.arange(1000), 1000, 0x9ABCDEF0, 0x9ABCDEF0))      # k0 matters
    assert not np.array_equal(a, np.arange(1000))
    assert [P.half_bits_of(n) for n in (1, 4, 5, 16, 17, 64, 65, 4097)] == [1, 1, 2, 2, 3, 3, 4, 7]


def test_u01_and_box_muller_edges():
    u = P.u01(np.array([0, 0xFF, 0x100, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32 and u[0] == 0.0 and u[1] == 0.0 and u[2] == np.float32(2.0 ** -24)
    assert u[3] == np.float32(1.0 - 2.0 ** -24) and (u >= 0).all() and (u < 1).all()
    z = np.zeros(1, dtype=np.uint32)
    g = P.box_muller((z, z, z, z), 1.0)
    assert g.shape == (1, 4) and np.isfinite(g).all()
    r = np.sqrt(-2.0 * np.log(2.0 ** -25))          # u1 = 0.5 * 2^-24, u2 = 0: (r, 0) twice -- the largest radius there is
    assert np.allclose(g[0], [r, 0.0, r, 0.0], rtol=0, atol=1e-15) and r < 5.9
    f = np.full(1, 0xFFFFFFFF, dtype=np.uint32)
    assert np.isfinite(P.box_muller((f, f, f, f), 2.0)).all()
    assert np.array_equal(P.gauss_noise(7, 1.0, 5), P.gauss_noise(8, 1.0, 5)[:7]) and P.gauss_noise(0, 1.0, 5).shape == (0,)


def test_epoch_rows_on_a_hand_made_plan():
    """Without the shuffle the source is the row; leaves with no rays are skipped; every pick lies in its leaf's ranges; the
    weighted picks land on pixels of the leaf's segment."""
    plan = np.array([[0, 0, 3, 0, 4, 0, 6], [0, 1, 0, 4, 8, 0, 6], [1, 0, 5, 2, 3, 5, 6]], dtype=np.int32)
    offs = np.array([0, 3, 3, 8], dtype=np.int64)
    src, leaf, pix = P.epoch_rows(plan, offs, 8, 77, False, 8, 6)
    assert np.array_equal(src, np.arange(8)) and leaf.tolist() == [0, 0, 0, 2, 2, 2, 2, 2]
    assert (pix[:3, 0] == 0).all() and (pix[:3, 1] < 4).all() and (pix[:3, 2] < 6).all() and (pix >= 0).all()
    assert np.array_equal(pix[3:], np.tile([1, 2, 5], (5, 1)))                # a one-pixel leaf
    s2, l2, p2 = P.epoch_rows(plan, offs, 8, 77, True, 8, 6)
    assert np.array_equal(np.sort(s2), np.arange(8)) and not np.array_equal(s2, src)
    assert np.array_equal(l2, leaf[s2]) and np.array_equal(p2, pix[s2])      # the pick is keyed by the source, not by the row
    wt = dict(n_weighted=[2, 0, 5], seg_beg=[0, 2, 2], seg_end=[2, 2, 3], order=[7, 13, 8 * 6 + 2 * 6 + 5],
              cum=np.array([1.0, 1.0 + 1e-9, 4.0]))
    _, _, p3 = P.epoch_rows(plan, offs, 8, 77, False, 8, 6, weighted=wt)
    assert all(tuple(p) in ((0, 1, 1), (0, 2, 1)) for p in p3[:2]) and np.array_equal(p3[2], pix[2])
    assert np.array_equal(p3[3:], pix[3:])


@pytest.mark.parametrize('world', [1, 2, 8])
def test_epoch_shard_rows_equals_the_listed_rows(world):
    from fastnerf import _lib, parallel
    lib = _lib.lib()
    for N in (0, 1, 7, 1000):
        for batch in (1, 5, 1000, 1920):
            tot = 0
            for rk in range(world):
                rows = parallel.shard_global_rows(N, batch, rk, world)
                assert int(lib.fastnerf_epoch_shard_rows(N, batch, rk, world)) == len(rows), (N, batch, rk, world)
                tot += len(rows)
            assert tot == N
    assert lib.fastnerf_epoch_shard_rows(10, 5, 8, 8) == -1 and lib.fastnerf_epoch_shard_rows(10, 0, 0, 1) == -1
