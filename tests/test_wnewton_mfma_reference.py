"""CPU proof for tests/test_gpu_wnewton_mfma.py: on the very inputs that test gives the matrix-core moments kernel
(sgdnet_amd/csrc/newton_mfma.hip, the option "wnewton_moments" = 1), one outer step restated in float64 with every sum taken
the way that kernel takes it -- four rows a matrix instruction, slab by slab, chunk by chunk -- passes the checks of
tests/wide_passes_reference.py, and a wrong version does not.  The shapes are the kernel's own edges, from its geometry
(csrc/wide_layout.hpp): T columns a macro tile, S rows a slab, C rows a chunk while the chunks are the shortest allowed."""
import numpy as np
import pytest

import newton_reference as N
import wide_passes_reference as W

T, S, C = 64, 32, 256
# p + 2 on either side of a 16-column tile and of a macro tile ("ones" and "r" in one, or apart), a diagonal pair alone and
# with an off-diagonal one; the rows around the instruction's depth of 4 and the slab; one, two and three chunks, the last
# holding one row.  (n, p); centring alternates with the index.
SHAPES = ([(48, nc - 2) for nc in (3, 15, 16, 17, T - 1, T, T + 1, T + 2, 2 * T + 1)] + [(n, 7) for n in (1, 3, 4, 5, S - 1, S, S + 1)]
          + [(n, 7) for n in (C, C + 1, 2 * C, 2 * C + 1)])
CASES = [(n, p, i % 2) for i, (n, p) in enumerate(SHAPES)]
PEN = dict(zip(("l2", "l1", "ridge"), W.MIX["mix0.5"]))


def row_chunks(n, ncols):
    """csrc/wide_layout.hpp: wide_mfma_row_chunks"""
    tiles = -(-ncols // T)
    pairs = tiles * (tiles + 1) // 2
    cap = 1 if pairs >= 2048 else 2048 // pairs
    rows = max(C, -(-(-(-n // cap)) // S) * S)
    return -(-n // rows), rows


def mfma_sum(t):
    """lane group g of a wavefront takes the rows 8 g + s of a slab in step s; a step adds its four products to the accumulator;
    the chunks' accumulators are added in chunk order"""
    t = np.asarray(t, dtype=np.float64)
    total = np.zeros(t.shape[1:])
    for c0 in range(0, len(t), C):
        chunk = t[c0:c0 + C]
        pad = np.zeros(((-len(chunk)) % S,) + t.shape[1:])
        acc = np.zeros(t.shape[1:])
        for slab in np.concatenate([chunk, pad]).reshape((-1, 4, 8) + t.shape[1:]):
            for s in range(8):
                acc = acc + ((slab[0, s] + slab[1, s]) + (slab[2, s] + slab[3, s]))
        total = total + acc
    return total


def test_the_shapes_sit_where_the_geometry_branches():
    assert [row_chunks(n, 9) for n in (C, C + 1, 2 * C, 2 * C + 1)] == [(1, C), (2, C), (2, C), (3, C)]
    assert all(row_chunks(n, p + 2)[1] == C for n, p in SHAPES)                 # mfma_sum's chunks are the kernel's
    assert row_chunks(20000, 1002) == (15, 1344) and row_chunks(500, 2002) == (2, C) and row_chunks(1 << 30, 5821)[0] == 1


@pytest.mark.parametrize("n,p,centre", CASES)
def test_the_kernels_order_stays_inside_and_a_wrong_version_does_not(n, p, centre):
    case = W.wn_case(n, p, centre)
    u = N.candidate(case, "moderate")
    W.wn_check_probe(W.wn_restate(case, u, 0.5, max_sweeps=1, fsum=mfma_sum, **PEN), case, u, 0.5, max_sweeps=1, **PEN)
    with pytest.raises(AssertionError):
        W.wn_check_probe(W.wn_restate(case, u, 0.5, max_sweeps=1, fsum=mfma_sum, wrong="wrong_triangle", **PEN), case, u, 0.5, max_sweeps=1, **PEN)
