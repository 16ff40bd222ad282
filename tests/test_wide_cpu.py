"""CPU: the argument contract of the wide-scorer entries (csrc/ltr_wide.hip) -- every rule is answered before any launch, so none of
this needs a device -- the buffer-size formulas of include/ltr_mi355x.h, and WideFusedRanker's refusals."""
import ctypes

import pytest
import torch

import wide_cases as WC

NULL, SHAPE, PARAM, ALIGN = -1, -2, -3, -4
RELU3, SIGMOID2 = 0, 1


@pytest.fixture(scope="module")
def handle():
    from ltr_mi355x.build import build
    build(force=False, verbose=False)
    import ltr_mi355x
    return ltr_mi355x.lib()


_BUF = (ctypes.c_char * 256)()
_A16 = (ctypes.addressof(_BUF) + 15) & ~15         # a 16-byte aligned address that is valid to pass and never dereferenced
_PARAMS = (ctypes.c_void_p * 6)(*([_A16] * 6))


def _p_code(p):
    from ltr_mi355x.scorer import drop_code
    return drop_code(True, p)


def _forward(h, **ch):
    a = dict(kind=RELU3, F=220, H1=220, H2=220, X=_A16, n_docs=8, params=_PARAMS, dropout=0, seed=0, keep1=None, keep2=None, scores=_A16,
             acts=_A16)
    a.update(ch)
    return h.ltr_wide_forward_save(a["kind"], a["F"], a["H1"], a["H2"], a["X"], a["n_docs"], a["params"], a["dropout"], a["seed"],
                                   a["keep1"], a["keep2"], a["scores"], a["acts"], None)


def _backward(h, **ch):
    a = dict(kind=RELU3, F=220, H1=220, H2=220, X=_A16, n_docs=8, params=_PARAMS, dropout=0, acts=_A16, dscores=_A16, ws=_A16, grid=8,
             flat=_A16)
    a.update(ch)
    return h.ltr_wide_backward_saved(a["kind"], a["F"], a["H1"], a["H2"], a["X"], a["n_docs"], a["params"], a["dropout"], a["acts"],
                                     a["dscores"], a["ws"], a["grid"], a["flat"], None)


def _some_null(k):
    ps = [_A16] * 6
    ps[k] = None
    return (ctypes.c_void_p * 6)(*ps)


_BAD_P = 1 | 0x40000000          # the drop code of p = 2.0

COMMON = [
    (dict(X=None), NULL), (dict(params=None), NULL), (dict(acts=None), NULL), (dict(params=_some_null(0)), NULL),
    (dict(params=_some_null(5)), NULL), (dict(kind=SIGMOID2, params=_some_null(3)), NULL),
    (dict(kind=SIGMOID2, params=_some_null(4)), None),        # the folded network has four tensors: entry 4 is not read
    (dict(F=0), SHAPE), (dict(F=1025), SHAPE), (dict(H1=0), SHAPE), (dict(H1=1025), SHAPE), (dict(H2=0), SHAPE), (dict(H2=1025), SHAPE),
    (dict(kind=SIGMOID2, H2=0), None),                          # H2 is ignored there
    (dict(n_docs=-1), SHAPE), (dict(kind=2), PARAM), (dict(kind=-1), PARAM), (dict(dropout=_BAD_P), PARAM),
    (dict(dropout=1 | 0x80000000), PARAM),                      # p = -0.0 with the dropout bit set
    (dict(X=_A16 + 4), ALIGN), (dict(acts=_A16 + 8), ALIGN),
    # two rules at once: the order NULL, SHAPE, PARAM, ALIGN, then the zero-size call
    (dict(X=None, F=0), NULL), (dict(F=0, kind=2), SHAPE), (dict(kind=2, X=_A16 + 4), PARAM), (dict(dropout=_BAD_P, acts=_A16 + 4), PARAM),
    (dict(n_docs=0, X=_A16 + 4), ALIGN), (dict(n_docs=0, kind=7), PARAM),
]


def test_forward_save_answers_before_any_launch(handle):
    for ch, code in COMMON + [(dict(scores=None), NULL), (dict(n_docs=0), 0), (dict(n_docs=0, dropout=1), 0),
                              (dict(n_docs=0, dropout=_p_code(0.3)), 0), (dict(n_docs=0, kind=SIGMOID2, H1=32), 0)]:
        if code is None:
            ch, code = dict(ch, n_docs=0), 0                    # a valid call: the zero-size form answers without a device
        assert _forward(handle, **ch) == code, ch


def test_backward_saved_answers_before_any_launch(handle):
    for ch, code in COMMON + [(dict(dscores=None), NULL), (dict(ws=None), NULL), (dict(flat=None), NULL), (dict(grid=0), SHAPE),
                              (dict(grid=65536), SHAPE), (dict(ws=_A16 + 4), ALIGN), (dict(grid=0, kind=3), SHAPE)]:
        if code is None:
            continue                                            # valid calls: the backward's zero-size form clears flat_grad on the device
        assert _backward(handle, **ch) == code, ch


def _gemm(h, **ch):
    from ltr_mi355x.wide import GemmDesc
    a = dict(A=_A16, B=_A16, C=_A16, M=8, N=8, K=8, lda=8, ldb=8, ldc=8, splits=1)
    a.update(ch)
    return h.ltr_gemm_f32(ctypes.byref(GemmDesc(**a)), None)


def test_gemm_and_colsum_answer_before_any_launch(handle):
    h = handle
    assert h.ltr_gemm_f32(None, None) == NULL
    for ch, code in [(dict(A=None), NULL), (dict(B=None), NULL), (dict(C=None), NULL), (dict(gate_kind=1), NULL),
                     (dict(M=-1), SHAPE), (dict(N=0), SHAPE), (dict(N=1025), SHAPE), (dict(K=0), SHAPE), (dict(splits=0), SHAPE),
                     (dict(splits=1025), SHAPE), (dict(lda=7), SHAPE), (dict(ldb=7), SHAPE), (dict(ldc=7), SHAPE),
                     (dict(a_kmajor=1, M=9), SHAPE), (dict(b_kmajor=1, N=9, ldc=9), SHAPE), (dict(gate=_A16, gate_kind=1, ldg=7), SHAPE),
                     (dict(act=3), PARAM), (dict(act=-1), PARAM), (dict(gate=_A16, gate_kind=3, ldg=8), PARAM), (dict(drop_layer=2), PARAM),
                     (dict(dropout=_BAD_P), PARAM), (dict(A=_A16 + 2), ALIGN), (dict(C=_A16 + 1), ALIGN), (dict(bias=_A16 + 3), ALIGN),
                     (dict(M=0), 0), (dict(M=0, A=_A16 + 4, lda=9), 0),            # a 4-byte aligned operand is accepted
                     (dict(A=None, N=0), NULL), (dict(N=0, act=3), SHAPE), (dict(act=3, A=_A16 + 2), PARAM), (dict(M=0, A=_A16 + 2), ALIGN)]:
        assert _gemm(h, **ch) == code, ch
    cs = lambda y=_A16, T=8, N=8, ld=8, w=None, parts=_A16, nblk=4: h.ltr_colsum_f32(y, T, N, ld, w, parts, nblk, None)     # noqa: E731
    assert cs(y=None) == NULL and cs(parts=None) == NULL
    for kw in (dict(T=-1), dict(N=0), dict(N=1025), dict(ld=7), dict(nblk=0), dict(nblk=65536)):
        assert cs(**kw) == SHAPE, kw
    assert cs(y=None, N=0) == NULL


@pytest.mark.parametrize("kind,F,H1,H2", [(RELU3, 137, 137, 137), (RELU3, 220, 220, 220), (RELU3, 700, 700, 700), (RELU3, 1024, 1024, 1024),
                                          (RELU3, 220, 64, 33), (SIGMOID2, 220, 32, 32), (SIGMOID2, 1024, 32, 0), (SIGMOID2, 137, 1, 5)])
def test_buffer_sizes_follow_the_header(handle, kind, F, H1, H2):
    for n in (0, 1, 3, 63, 64, 65, 185, 4736, 200000):
        assert handle.ltr_wide_acts_floats(kind, F, H1, H2, n) == WC.acts_floats(kind, F, H1, H2, n)
        for grid in (1, 8, 256, 512, 65535):
            assert handle.ltr_wide_ws_floats(kind, F, H1, H2, n, grid) == WC.ws_floats(kind, F, H1, H2, n, grid), (n, grid)


def test_buffer_sizes_reject_bad_shapes(handle):
    h = handle
    for fn, tail in ((h.ltr_wide_acts_floats, ()), (h.ltr_wide_ws_floats, (8,))):
        assert fn(RELU3, 0, 8, 8, 4, *tail) == SHAPE and fn(RELU3, 1025, 8, 8, 4, *tail) == SHAPE
        assert fn(RELU3, 8, 0, 8, 4, *tail) == SHAPE and fn(RELU3, 8, 8, 1025, 4, *tail) == SHAPE
        assert fn(RELU3, 8, 8, 8, -1, *tail) == SHAPE and fn(SIGMOID2, 8, 1025, 8, 4, *tail) == SHAPE
        assert fn(2, 8, 8, 8, 4, *tail) == PARAM and fn(2, 0, 8, 8, 4, *tail) == SHAPE
    assert h.ltr_wide_ws_floats(RELU3, 8, 8, 8, 4, 0) == SHAPE and h.ltr_wide_ws_floats(RELU3, 8, 8, 8, 4, 65536) == SHAPE


def test_wide_ranker_refusals():
    from architeture.doubleLayer import DoubleLayerNet
    from architeture.tripleLayer import TripleLayerNet
    from ltr_mi355x import LtrDeviceError
    from ltr_mi355x.scorer import FusedRanker
    from ltr_mi355x.wide import WideFusedRanker
    assert WideFusedRanker.LOSSES.keys() == FusedRanker.LOSSES.keys() and WideFusedRanker.LOSSES == FusedRanker.LOSSES
    for cls in (DoubleLayerNet, TripleLayerNet):
        with pytest.raises(LtrDeviceError):
            WideFusedRanker(cls(220))                           # CPU tensors: no fallback
        with pytest.raises(ValueError, match="FusedRanker"):
            WideFusedRanker(cls(136))
        with pytest.raises(ValueError, match="1024"):
            WideFusedRanker(cls(1025))
        with pytest.raises(KeyError):
            WideFusedRanker(cls(220), loss="no_such_loss")
        with pytest.raises(TypeError, match="risk_args"):
            WideFusedRanker(cls(220), loss="listnet", risk_args={"alpha": 2.0})
    with pytest.raises(TypeError):
        WideFusedRanker(torch.nn.Linear(220, 1))
    with pytest.raises(NotImplementedError, match="136"):       # FusedRanker itself keeps refusing these widths
        FusedRanker(DoubleLayerNet(220))
