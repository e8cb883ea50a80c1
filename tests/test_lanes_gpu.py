"""The cross-lane primitives of csrc/sco_lanes.h, one at a time on one wavefront (sco_debug_lanes, csrc/sco_lanes_probe.hip),
bit for bit against a numpy model.

The model is written from what the hardware does to lane indices, not from the header: a DPP control names a source lane
for every lane (row_shr:n lane l - n of the same 16-lane row, quad_perm [1,0,3,2] lane l ^ 1, [2,3,0,1] l ^ 2,
row_half_mirror l ^ 7, row_mirror l ^ 15, row_bcast15 / row_bcast31 lane 15 of the row below / lane 31); a lane without a
source, or in a row the row mask leaves out, gets zero or keeps its own value; v_permlane32_swap exchanges the upper 32
lanes of a with the lower 32 of b, v_permlane16_swap the odd rows of a with the even rows of b.  The reductions compose
these in the step order the header documents.  float64 addition and fmax of numpy are IEEE, as on the GPU, so a changed
association order shows in the 2^53-scale vector and a lost or invented NaN in the NaN vectors.

Scans promise lane 15 of every row, or lane 63, and only those lanes are compared; everything else promises all 64."""
import numpy as np
import pytest

from sco_py_amd import _lib

pytestmark = pytest.mark.gpu

L = np.arange(64)
ROW = L >> 4
ALL = L
LANE15 = L[(L & 15) == 15]
LANE63 = L[63:]


# ---- what the hardware does to lane indices --------------------------------------------------------------------------
def _dpp(v, src, has_src, keep):
    return np.where(has_src, v[np.where(has_src, src, L)], v if keep else 0.0)


def _xor(k):
    return lambda v, keep=False: _dpp(v, L ^ k, L >= 0, keep)


def _shr(n):
    return lambda v, keep=False: _dpp(v, L - n, (L & 15) >= n, keep)


def _bcast15(v, keep=False):        # row mask 0xa: rows 1 and 3
    return _dpp(v, 16 * ROW - 1, (ROW == 1) | (ROW == 3), keep)


def _bcast31(v, keep=False):        # row mask 0xc: rows 2 and 3
    return _dpp(v, np.full(64, 31), ROW >= 2, keep)


def _swap(w, a, b):
    moved = (L >= 32) if w == 32 else (ROW & 1) == 1        # lanes of a that leave; they land w lanes lower in b
    return np.where(moved, b[(L - w) % 64], a), np.where(moved, b, a[(L + w) % 64])


def _op(is_max):
    return np.fmax if is_max else np.add


# ---- the primitives, composed in their documented order --------------------------------------------------------------
def _fold(w, is_max):
    return lambda a, b: (_op(is_max)(*_swap(w, a, b)), b)


def _step(move, is_max):
    return lambda v: _op(is_max)(v, move(v, keep=is_max))


def _chain(*steps):
    def run(v):
        for s in steps:
            v = s(v)
        return v
    return run


def _row15(is_max):
    return _chain(*[_step(_shr(n), is_max) for n in (1, 2, 4, 8)])


def _wave63(is_max):
    return _chain(_row15(is_max), _step(_bcast15, is_max), _step(_bcast31, is_max))


def _all_lanes(is_max):
    def run(v):
        for k in (1, 2, 7, 15):
            v = _op(is_max)(v, _xor(k)(v))
        v = _fold(16, is_max)(v, v)[0]
        return _fold(32, is_max)(v, v)[0]
    return run


def _shuffles(is_max):
    return _chain(*[(lambda v, o=o: _op(is_max)(v, v[L ^ o])) for o in (32, 16, 8, 4, 2, 1)])


def _one(f):
    return lambda a, b: (f(a), b)


# op number of sco_debug_lanes -> (name, model of (a, b) -> (out_a, out_b), lanes of out_a that are specified, out_b too)
OPS = {
    0: ("dpp quad_perm [1,0,3,2]", _one(_xor(1)), ALL, False),
    1: ("dpp quad_perm [2,3,0,1]", _one(_xor(2)), ALL, False),
    2: ("dpp row_half_mirror", _one(_xor(7)), ALL, False),
    3: ("dpp row_mirror", _one(_xor(15)), ALL, False),
    4: ("dpp row_shr:1, zero", _one(_shr(1)), ALL, False),
    5: ("dpp row_shr:8, own value", _one(lambda v: _shr(8)(v, keep=True)), ALL, False),
    6: ("dpp row_bcast15 on 0xa, zero", _one(_bcast15), ALL, False),
    7: ("dpp row_bcast31 on 0xc, own value", _one(lambda v: _bcast31(v, keep=True)), ALL, False),
    8: ("broadcast of lane 23", _one(lambda v: np.full(64, v[23])), ALL, False),
    9: ("swap 16", lambda a, b: _swap(16, a, b), ALL, True),
    10: ("swap 32", lambda a, b: _swap(32, a, b), ALL, True),
    11: ("fold 16 sum", _fold(16, False), ALL, False),
    12: ("fold 16 max", _fold(16, True), ALL, False),
    13: ("fold 32 sum", _fold(32, False), ALL, False),
    14: ("fold 32 max", _fold(32, True), ALL, False),
    15: ("scan step row_shr:2 sum", _one(_step(_shr(2), False)), ALL, False),
    16: ("scan step row_shr:4 max", _one(_step(_shr(4), True)), ALL, False),
    17: ("row scan sum", _one(_row15(False)), LANE15, False),
    18: ("row scan max", _one(_row15(True)), LANE15, False),
    19: ("wavefront scan sum", _one(_wave63(False)), LANE63, False),
    20: ("wavefront scan max", _one(_wave63(True)), LANE63, False),
    21: ("pair sum", _one(_step(_xor(1), False)), ALL, False),
    22: ("quad sum", _one(_chain(_step(_xor(1), False), _step(_xor(2), False))), ALL, False),
    23: ("all lanes sum", _one(_all_lanes(False)), ALL, False),
    24: ("all lanes max", _one(_all_lanes(True)), ALL, False),
    25: ("shuffle sum", _one(_shuffles(False)), ALL, False),
    26: ("shuffle max", _one(_shuffles(True)), ALL, False),
    27: ("reversal through LDS behind the fence", _one(lambda v: v[63 - L]), ALL, False),
}


def _inputs():
    rng = np.random.default_rng(20)
    ints_a = rng.permutation(2.0 * L - 63.0)                  # the odd integers -63 .. 63: distinct, no zero, both signs
    ints_b = rng.permutation(2.0 * L - 63.0) * 128.0
    big = 2.0 ** 53

    def mixed():       # 2^53 + 1 rounds back to 2^53, 2^53 + (1 + 1) does not: which small values meet first decides the bits
        v = rng.integers(1, 8, 64).astype(float) * rng.choice([-1.0, 1.0], 64)
        at = rng.random(64) < 0.3
        return np.where(at, np.sign(v) * big, v)

    one_a, one_b = ints_a.copy(), ints_b.copy()
    one_a[0] = np.nan                                         # lane 0: no source under any row_shr, row 0 under no broadcast
    one_b[32] = np.nan
    return {"integers": (ints_a, ints_b), "mixed scales": (mixed(), mixed()), "one NaN": (one_a, one_b),
            "all NaN": (np.full(64, np.nan), np.full(64, np.nan))}


INPUTS = _inputs()


def _same_bits(got, want, lanes, tag):
    g, w = got[lanes], want[lanes]
    assert np.array_equal(np.isnan(g), np.isnan(w)), (tag, "NaN positions", g, w)
    num = ~np.isnan(w)
    assert np.array_equal(g[num].view(np.int64), w[num].view(np.int64)), (tag, g, w)


def _run(op, a, b):
    out_a, out_b = np.full(64, -7.0), np.full(64, -7.0)
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    _lib.check(_lib.load().sco_debug_lanes(0, op, _lib.dptr(a), _lib.dptr(b), _lib.dptr(out_a), _lib.dptr(out_b)))
    return out_a, out_b


@pytest.mark.parametrize("op", sorted(OPS), ids=lambda k: OPS[k][0].replace(" ", "_"))
def test_primitive_matches_its_lane_contract(gpu, op):
    name, model, lanes, both = OPS[op]
    for tag, (a, b) in INPUTS.items():
        want_a, want_b = model(a, b)
        got_a, got_b = _run(op, a, b)
        _same_bits(got_a, want_a, lanes, (name, tag, "a"))
        if both:
            _same_bits(got_b, want_b, ALL, (name, tag, "b"))


def test_the_mixed_vector_tells_association_orders_apart():
    """The input meant to catch a changed summation order does.  The wavefront scan and the all-lanes sum are the same
    tree (neighbours first, halves last; addition commutes), the shuffles go the other way (halves first) and a plain
    loop is a third order: on this vector the three differ, for both operands."""
    for a in INPUTS["mixed scales"]:
        tree, shuffles, loop = _wave63(False)(a)[63], _shuffles(False)(a)[0], float(np.sum(a[::-1]))
        assert _all_lanes(False)(a)[0] == tree
        assert len({tree, shuffles, loop}) == 3, (tree, shuffles, loop)


def test_bad_arguments_are_refused(gpu):
    lib = _lib.load()
    a = np.zeros(64)
    assert lib.sco_debug_lanes(0, len(OPS), _lib.dptr(a), None, _lib.dptr(a), None) != 0
    assert lib.sco_debug_lanes(0, -1, _lib.dptr(a), None, _lib.dptr(a), None) != 0
    assert lib.sco_debug_lanes(0, 0, None, None, _lib.dptr(a), None) != 0
    assert lib.sco_debug_lanes(99, 0, _lib.dptr(a), None, _lib.dptr(a), None) != 0
