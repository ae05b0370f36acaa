"""The sizes include/fastnerf.h publishes against the library's own, and the layout of the folded view layer inside the packed forward
buffer (csrc/mlp_layout.h PFM | PFB | PFR, appended behind the ten older blocks).  Host only: size queries, no compute calls."""
import os
import re

import pytest

from fastnerf import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# kind: (PFM, PFB, PFR, pf_total) in floats of the fp32 packing; PFM is where the packed forward buffer ended before the fold moved in
LAYOUT = {0: (593920, 630784, 630912, 663680), 1: (593920, 630784, 630912, 663680), 2: (610304, 647168, 647296, 680064)}
FOLD_UNITS = (288 * 128, 128, 128 * 256)      # [M | Wv[:, 256:]] block, b', M row-major


def header_constants():
    src = open(os.path.join(ROOT, 'include', 'fastnerf.h')).read()
    return {k: int(v) for k, v in re.findall(r'^#define\s+(FASTNERF_\w+)\s+(\d+)\b', src, flags=re.M)}


def test_header_constants_are_the_librarys():
    c, lib = header_constants(), _lib.lib()
    assert c['FASTNERF_NET_PARAMS'] == lib.fastnerf_net_floats(0, 0)
    assert c['FASTNERF_PACKED_FWD'] == lib.fastnerf_net_floats(0, 1)
    assert c['FASTNERF_PACKED_BWD'] == lib.fastnerf_net_floats(0, 2)
    for P in (1, 1000):
        assert lib.fastnerf_mlp_act_floats(0, P) == P * c['FASTNERF_ACT_FLOATS'] + c['FASTNERF_ACT_SLACK']


@pytest.mark.parametrize('kind', [0, 1, 2])
def test_fold_regions_are_the_tail_of_packed_fwd(kind):
    lib = _lib.lib()
    pfm, pfb, pfr, total = LAYOUT[kind]
    off = [lib.fastnerf_mlp_fold_offset(kind, w) for w in range(3)]
    assert off == [pfm, pfb, pfr]
    assert lib.fastnerf_net_floats(kind, 1) == total
    # disjoint, back to back, from the old end of the buffer to the new one
    spans = sorted((o, o + n) for o, n in zip(off, FOLD_UNITS))
    assert spans[0][0] == pfm == total - sum(FOLD_UNITS)
    assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert spans[-1][1] == total
    assert all(o % 128 == 0 for o in off + [total])      # off * 3 / 2 and off * 3 / 8 exact, 16-byte aligned
    assert lib.fastnerf_mlp_x6_packed_floats(kind, 1) * 2 == total * 3
    assert lib.fastnerf_mlp_fold_offset(kind, 3) == 557056
    assert lib.fastnerf_net_floats(kind, 2) == 557056 + 128 * 256
    assert lib.fastnerf_mlp_fold_offset(kind, 4) == -1
