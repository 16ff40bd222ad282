"""The risk tails and the risk-matrix rows (csrc/ltr_risk.hip) against the fp64 oracle, at their edges.

Cases, inputs and preconditions come from tests/risk_tail_cases.py (checked on the CPU by test_risk_tails_cpu.py).  Everything goes
through the C ABI (ctypes).  Every comparison is against the fp64 oracle on the same fp32 inputs (oracle/ltr_risk_oracle.py:
risk_tail, t_risk_pair_tail, risk_closed_form, t_risk_tail; oracle/ltr_metrics_oracle.py for the zero-guard flavour), or is bit
equality between two forms that include/ltr_mi355x.h declares equal (blocks == dense, forward-only == forward + backward, cached ==
uncached).  No kernel of ltr_risk.hip serves as a reference.

Bar: max|delta| / max|ref| <= max(1e-5, 4 x the oracle's own fp32-vs-fp64 deviation on the same inputs); every compared
quantity goes to the parity ledger.  One allowance on top, for return strategies 2 / 3 (risk_tail_cases.rounding_allowance): the kernel
rounds R0 and R1 to fp32 before combining them, deliberately, where the reference does; one fp32 ulp of max(|R0|, |R1|) propagated
through the combination is added to the bar, with R0 and R1 taken from the fp64 oracle.
"""
import ctypes

import numpy as np
import pytest
import torch

import ltr_metrics_oracle as MO
import ltr_risk_oracle as RO
import risk_tail_cases as C
from conftest import ledger_record, relerr

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()           # fail loudly if the HIP library is missing
    return torch.device("cuda:0")


def _h():
    from ltr_mi355x._lib import lib
    return lib()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    from ltr_mi355x.functional import _stream as s
    return s()


def _check(rc, what):
    from ltr_mi355x._lib import check
    check(rc, what)


def gate(quantity, got, ref, ref32, what, extra=0.0):
    """Record and assert one quantity: err against the fp64 oracle, noise = the fp32 oracle against the fp64 oracle; `extra` is the
    strategy-2 / 3 rounding allowance (0 elsewhere)."""
    got, ref, ref32 = (np.asarray(t.detach().cpu().double().numpy() if isinstance(t, torch.Tensor) else t, dtype=np.float64)
                       for t in (got, ref, ref32))
    assert got.shape == ref.shape, (quantity, got.shape, ref.shape)
    assert bool(np.isfinite(got).all()), (quantity, what)
    err, noise = relerr(got, ref), relerr(ref32, ref)
    bar = max(TOL, 4.0 * noise) + extra
    ledger_record(quantity, err, noise=noise, tol=TOL, note=what if extra == 0.0 else f"{what} (+{extra:.2e} fp32 rounding of R0 / R1)")
    print(f"{what} {quantity}: rel_err {err:.3e} oracle fp32 noise {noise:.3e} bar {bar:.3e}")
    assert err <= bar, (quantity, what, err, noise, extra)


# ------------------------------------------------------------------------------------------------- launches
def risk_tail(md, o, grad=True):
    """ltr_risk_tail_fwd_bwd on a device matrix [Q, n]: (value [1], dmat or None), both NaN-filled before the launch."""
    Q, n = md.shape
    value = torch.full((1,), NAN, dtype=torch.float32, device=md.device)
    dmat = torch.full((Q, n), NAN, dtype=torch.float32, device=md.device) if grad else None
    _check(_h().ltr_risk_tail_fwd_bwd(_p(md), Q, n, o.alpha, int(o.geo), o.strategy, int(o.flip), o.factor, int(o.zquirk), _p(value),
                                      _p(dmat), _stream()), "ltr_risk_tail_fwd_bwd")
    return value, dmat


def trisk_tail(md, o, grad=True):
    Q = md.shape[0]
    value = torch.full((1,), NAN, dtype=torch.float32, device=md.device)
    dmat = torch.full((Q, 2), NAN, dtype=torch.float32, device=md.device) if grad else None
    _check(_h().ltr_trisk_tail_fwd_bwd(_p(md), Q, o.alpha, int(o.flip), o.factor, _p(value), _p(dmat), _stream()), "ltr_trisk_tail_fwd_bwd")
    return value, dmat


def tail_blocks(bd, lay, n, o, grad=True):
    """The blocks form of either tail; dmat (the blocks' layout) is CANARY-filled before the launch."""
    value = torch.full((1,), NAN, dtype=torch.float32, device=bd.device)
    dmat = torch.full(tuple(bd.shape), C.CANARY, dtype=torch.float32, device=bd.device) if grad else None
    if isinstance(o, C.TOpt):
        _check(_h().ltr_trisk_tail_blocks_fwd_bwd(_p(bd), lay.n_blocks, lay.block_rows, o.alpha, int(o.flip), o.factor, _p(value), _p(dmat),
                                                  _stream()), "ltr_trisk_tail_blocks_fwd_bwd")
    else:
        _check(_h().ltr_risk_tail_blocks_fwd_bwd(_p(bd), lay.n_blocks, lay.block_rows, n, o.alpha, int(o.geo), o.strategy, int(o.flip),
                                                 o.factor, int(o.zquirk), _p(value), _p(dmat), _stream()), "ltr_risk_tail_blocks_fwd_bwd")
    return value, dmat


def oracle_tail(m, o, dtype):
    """(value [1], d value / d mat, R0, R1) of the oracle in `dtype` on the fp32 matrix m."""
    x = m.detach().clone().to(dtype).requires_grad_(True)
    if isinstance(o, C.TOpt):
        val, r0, r1 = RO.t_risk_pair_tail(x, o.alpha, o.flip, o.factor), None, None
    else:
        val, r0, r1 = RO.risk_tail_parts(x, o.alpha, o.geo, o.strategy, o.flip, o.factor, o.zquirk)
    g, = torch.autograd.grad(val.sum(), x)
    return val.detach(), g, None if r0 is None else float(r0.detach()), None if r1 is None else float(r1.detach())


def tail_name(o):
    if isinstance(o, C.TOpt):
        return f"trisk_tail.{'flip' if o.flip else 'noflip'}"
    return f"risk_tail.{'geo' if o.geo else 'z'}.s{o.strategy}{'q' if o.zquirk else ''}.{'flip' if o.flip else 'noflip'}"


# ------------------------------------------------------------------------------------------------- dense tails
@pytest.mark.parametrize("Q,n,variant", C.tail_shapes(), ids=lambda v: str(v))
def test_risk_tail_against_the_oracle(Q, n, variant, dev):
    """ltr_risk_tail_fwd_bwd, every option set, value and d value / d mat against the fp64 oracle on the same fp32 matrix.  Bar:
    max(1e-5, 4 x noise) + the rounding allowance of strategies 2 / 3 (formula: risk_tail_cases.rounding_allowance -- u = one fp32 ulp
    of max(|R0|, |R1|) from the fp64 oracle; strategy 2 value u / |value|, strategy 3 value 2 u / |R1 - R0|, strategy 3 gradient
    u / |R1 - R0|).  With max ties the gradient equals the oracle's (torch's max splits evenly among ties) and the sum of dmat over
    the tied entries carries exactly the flip's share.  Where every residual is 0 up to rounding (equal rows, one query, one system)
    the value is compared absolutely and the gradient is not compared."""
    m = C.matrix(variant, Q, n)
    md = m.to(dev)
    ties = C.tie_positions(variant, Q, n)
    tr, tc = torch.tensor([r for r, _ in ties], dtype=torch.long), torch.tensor([c for _, c in ties], dtype=torch.long)
    for o in C.options():
        what = f"Q{Q}-n{n}-{variant}-{C.opt_id(o)}"
        value, dmat = risk_tail(md, o)
        v64, g64, r0, r1 = oracle_tail(m, o, torch.float64)
        if C.expect_nan(variant, n, o):                               # 0 / 0 on both sides, and nothing else asserted
            assert bool(torch.isnan(value).all()) and bool(torch.isnan(v64).all()), what
            continue
        assert bool(torch.isfinite(v64).all()) and bool(torch.isfinite(g64).all()), what
        assert bool(torch.isfinite(value).all()) and bool(torch.isfinite(dmat).all()), what
        if C.absolute(variant, Q, n):
            assert abs(float(value) - float(v64)) < 1e-5, (what, float(value), float(v64))
            continue
        v32, g32, _, _ = oracle_tail(m, o, torch.float32)
        # strategies 2 / 3: + one fp32 ulp of max(|R0|, |R1|) through the combination (R0, R1, value from the fp64 oracle)
        extra_v, extra_g = C.rounding_allowance(o, r0, r1, float(v64)) if o.strategy > 1 else (0.0, 0.0)
        gate(f"{tail_name(o)}.value [{C.q_regime(Q)}]", value, v64, v32, what, extra_v)
        gate(f"{tail_name(o)}.dmat [{C.q_regime(Q)}]", dmat, g64, g32, what, extra_g)
        if ties and o.flip:
            # the flip's share: with x' = -x + max(x) a leaf, d value / d x = -g' + [x is maximal] sum(g') / ties, so the tied
            # entries' gradients sum to sum(g') - (the sum of g' over them) -- from an oracle run that never differentiates a max.
            # A sum of len(ties) gradient entries: compared on the scale len(ties) max|gradient|, where the gradient's bar carries over.
            def share(dtype):
                xf = (-m.to(dtype) + m.to(dtype).max()).requires_grad_(True)
                val = RO.risk_tail(xf, o.alpha, o.geo, o.strategy, False, o.factor, o.zquirk)
                gp, = torch.autograd.grad(val.sum(), xf)
                return (gp.sum() - gp[tr, tc].sum()).double(), (len(ties) * gp.abs().max()).double()
            s64, s32 = torch.stack(share(torch.float64)), torch.stack(share(torch.float32))
            got = torch.stack([dmat.cpu()[tr, tc].double().sum(), s64[1]])
            gate(f"{tail_name(o)}.tie_share [{C.q_regime(Q)}]", got, s64, s32, what, extra_g)


@pytest.mark.parametrize("Q,variant", C.t_shapes(), ids=lambda v: str(v))
def test_trisk_tail_against_the_oracle(Q, variant, dev):
    """ltr_trisk_tail_fwd_bwd on [Q, 2], every option set, against RO.t_risk_pair_tail in fp64."""
    m = C.matrix(variant, Q, 2)
    md = m.to(dev)
    for o in C.t_options():
        what = f"Q{Q}-{variant}-{C.opt_id(o)}"
        value, dmat = trisk_tail(md, o)
        v64, g64, _, _ = oracle_tail(m, o, torch.float64)
        v32, g32, _, _ = oracle_tail(m, o, torch.float32)
        gate(f"{tail_name(o)}.value [{C.q_regime(Q)}]", value, v64, v32, what)
        gate(f"{tail_name(o)}.dmat [{C.q_regime(Q)}]", dmat, g64, g32, what)


def test_trisk_tail_of_one_query_is_nan_on_both_sides(dev):
    m = torch.tensor([[0.3, 0.5]])
    o = C.TOpt(False, 5.0, 1.0)
    value, _ = trisk_tail(m.to(dev), o)
    assert bool(torch.isnan(value).all()) and bool(torch.isnan(RO.t_risk_pair_tail(m.double(), 5.0, False, 1.0)).all())


# ------------------------------------------------------------------------------------------------- blocks forms
BLOCK_OPTS = (C.Opt(True, 1, False, True, 5.0, 1.0), C.Opt(True, 3, False, True, 1.0, -1.0), C.Opt(False, 2, True, False, 5.0, -1.0),
              C.Opt(False, 3, False, True, 0.0, 1.0), C.TOpt(True, 5.0, -1.0), C.TOpt(False, 1.0, 1.0))


@pytest.mark.parametrize("Q", C.BLOCK_Q)
def test_blocks_forms_are_the_dense_launch_bit_for_bit(Q, dev):
    """ltr_risk_tail_blocks_fwd_bwd / ltr_trisk_tail_blocks_fwd_bwd on every layout of risk_tail_cases.layouts(Q): value and the
    valid rows of dmat are torch.equal to the dense launch on the same rows (the header's "same bits"), with NaN padding and with
    finite padding; headers and padding of dmat keep their canary; the input blocks (counts included) are untouched.  The tied
    maxima of max_ties_third make the tie pass run through the block row map."""
    for o in BLOCK_OPTS:
        t = isinstance(o, C.TOpt)
        for n in ((2,) if t else (3, 9) if Q == 1025 else (3,)):
            m = C.matrix("max_ties_third", Q, n)
            md = m.to(dev)
            v_dense, g_dense = (trisk_tail if t else risk_tail)(md, o)
            assert bool(torch.isfinite(v_dense).all()) and bool(torch.isfinite(g_dense).all())
            for lay in C.layouts(Q):
                mask = C.padding_mask(lay, n).to(dev)
                for pad in (NAN, 3.0e30):
                    what = f"Q{Q}-n{n}-{lay.name}-pad{pad}-{C.opt_id(o)}"
                    b = C.pack(m, lay, pad)
                    bd = b.to(dev)
                    value, dmat = tail_blocks(bd, lay, n, o)
                    assert torch.equal(value, v_dense), (what, float(value), float(v_dense))
                    assert torch.equal(C.unpack_like(dmat.cpu(), b, n), g_dense.cpu()), what
                    assert bool((dmat[mask] == C.CANARY).all()), what
                    back = bd.cpu()
                    assert torch.equal(back[:, 0], b[:, 0]) and torch.equal(C.unpack(back, n), m), what
                    v_only, _ = tail_blocks(bd, lay, n, o, grad=False)                       # dmat = NULL: same value bits
                    assert torch.equal(v_only, v_dense), what


@pytest.mark.parametrize("Q", [1025, 2049])
def test_blocks_forms_against_the_oracle(Q, dev):
    """The pair (blocks, dense) is not only self-consistent: the straddling layout against the fp64 oracle directly."""
    for o in (C.Opt(True, 3, False, True, 5.0, -1.0), C.TOpt(True, 5.0, 1.0)):
        n = 2 if isinstance(o, C.TOpt) else 3
        m = C.matrix("max_ties_third", Q, n)
        lay = [x for x in C.layouts(Q) if x.name == "block_straddles_row_1024"][0]
        b = C.pack(m, lay)
        value, dmat = tail_blocks(b.to(dev), lay, n, o)
        v64, g64, r0, r1 = oracle_tail(m, o, torch.float64)
        v32, g32, _, _ = oracle_tail(m, o, torch.float32)
        ev, eg = (0.0, 0.0) if r0 is None else C.rounding_allowance(o, r0, r1, float(v64))
        what = f"Q{Q}-{lay.name}-{C.opt_id(o)}"
        gate(f"{tail_name(o)}.blocks.value", value, v64, v32, what, ev)
        gate(f"{tail_name(o)}.blocks.dmat", C.unpack_like(dmat.cpu(), b, n), g64, g32, what, eg)


@pytest.mark.parametrize("Q", [3, 65, 1025, 4097])
def test_forward_only_gives_the_same_value_bits(Q, dev):
    """dmat = NULL: the value of both dense tails is bitwise the value of the forward + backward launch, every option set."""
    m3, m2 = C.matrix("max_ties_third", Q, 3).to(dev), C.matrix("plain", Q, 2).to(dev)
    for o in C.options():
        assert torch.equal(risk_tail(m3, o, grad=False)[0], risk_tail(m3, o)[0]), C.opt_id(o)
    for o in C.t_options():
        assert torch.equal(trisk_tail(m2, o, grad=False)[0], trisk_tail(m2, o)[0]), C.opt_id(o)


# ------------------------------------------------------------------------------------------------- per-column kernels
@pytest.mark.parametrize("Q", [1023, 1024, 1025, 2049])
def test_per_column_kernels_past_one_sweep(Q, dev):
    """ltr_risk_fwd_bwd against RO.risk_closed_form, ltr_trisk_fwd_bwd against RO.t_risk_tail (autograd), both in fp64; and the
    LTR_RISK_ZERO_GUARD flavour on a matrix with two all-zero rows against MO.geo_risk_all_systems (numpy fp64: its noise is 0)."""
    h, n = _h(), 4
    m = C.matrix("plain", Q, n)
    md = m.to(dev)
    for geo in (False, True):
        for alpha in (1.0, 5.0):
            for col in (0, 1, -1):
                value = torch.full((1,), NAN, dtype=torch.float32, device=dev)
                dmat = torch.full((Q, n), NAN, dtype=torch.float32, device=dev)
                _check(h.ltr_risk_fwd_bwd(_p(md), Q, n, col, alpha, int(geo), _p(value), _p(dmat), _stream()), "ltr_risk_fwd_bwd")
                v64, g64 = RO.risk_closed_form(m.double(), alpha, col, geo)
                v32, g32 = RO.risk_closed_form(m, alpha, col, geo)
                what = f"Q{Q}-{'geo' if geo else 'z'}-a{alpha:g}-col{col}"
                gate(f"risk_fwd_bwd.{'geo' if geo else 'z'}.value", value, v64.reshape(1), v32.reshape(1), what)
                gate(f"risk_fwd_bwd.{'geo' if geo else 'z'}.dmat", dmat, g64, g32, what)
    for alpha in (0.0, 5.0):
        def trisk(dtype):
            a, b = m[:, 0].to(dtype).requires_grad_(True), m[:, 1].to(dtype).requires_grad_(True)
            v = RO.t_risk_tail(a, b, alpha)
            ga, gb = torch.autograd.grad(v, (a, b))
            return v.detach().reshape(1), ga, gb
        a, b = md[:, 0].contiguous(), md[:, 1].contiguous()
        value, da, db = (torch.full(s, NAN, dtype=torch.float32, device=dev) for s in ((1,), (Q,), (Q,)))
        _check(h.ltr_trisk_fwd_bwd(_p(a), _p(b), Q, alpha, _p(value), _p(da), _p(db), _stream()), "ltr_trisk_fwd_bwd")
        (v64, a64, b64), (v32, a32, b32) = trisk(torch.float64), trisk(torch.float32)
        gate("trisk_fwd_bwd.value", value, v64, v32, f"Q{Q}-a{alpha:g}")
        gate("trisk_fwd_bwd.dmodel", da, a64, a32, f"Q{Q}-a{alpha:g}")
        gate("trisk_fwd_bwd.dbaseline", db, b64, b32, f"Q{Q}-a{alpha:g}")
    z = m.clone()
    z[1] = 0.0
    z[Q - 1] = 0.0
    zd = z.to(dev)
    for alpha in (1.0, 5.0):
        want = MO.geo_risk_all_systems(z.numpy(), alpha)
        got = []
        for col in range(n):
            value = torch.full((1,), NAN, dtype=torch.float32, device=dev)
            _check(h.ltr_risk_fwd_bwd(_p(zd), Q, n, col, alpha, 1 | 4, _p(value), None, _stream()), "ltr_risk_fwd_bwd")   # GEO | ZERO_GUARD
            got.append(float(value))
        gate("risk_fwd_bwd.geo_zero_guard.value", np.array(got), want, want, f"Q{Q}-a{alpha:g}")


# ------------------------------------------------------------------------------------------------- matrix rows
def matrix_launch(ref, x0, rest, mode, lt, ideal, entry, dev):
    """(mat, jac) of ltr_risk_matrix_fwd (entry "fwd") or ltr_risk_matrix_rows_fwd with ones = 1 (entry "rows"), NaN-filled before."""
    h = _h()
    B, S = x0.shape
    nr = 0 if rest is None else (rest.shape[0] if mode == 1 else rest.shape[2])
    ld = 1 + nr + int(ideal) + (entry == "rows")
    mat = torch.full((B, ld), NAN, dtype=torch.float32, device=dev)
    jac = torch.full((B, S), NAN, dtype=torch.float32, device=dev)
    rd, xd, sd = ref.to(dev), x0.to(dev), None if rest is None else rest.to(dev).contiguous()
    if entry == "rows":
        _check(h.ltr_risk_matrix_rows_fwd(_p(rd), _p(xd), _p(sd), B, S, nr, mode, lt, int(ideal), 1, _p(mat), _p(jac), _stream()),
               "ltr_risk_matrix_rows_fwd")
    else:
        _check(h.ltr_risk_matrix_fwd(_p(rd), _p(xd), _p(sd), B, S, nr, mode, lt, int(ideal), _p(mat), _p(jac), _stream()), "ltr_risk_matrix_fwd")
    return mat, jac


@pytest.mark.parametrize("S", C.MATRIX_S)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_matrix_rows_against_the_oracle(S, mode, dev):
    """ltr_risk_matrix_fwd and ltr_risk_matrix_rows_fwd (ones = 1: one more column of exactly 1.0) at B = 3, lt 1..3, n_rest 0 / 1 / 3,
    ideal off / on: the matrix and jac = d mat[:, 0] / d x0 against risk_tail_cases.matrix_oracle in fp64 (autograd); modes 0 / 2 also
    through ltr_risk_matrix_cached_fwd, torch.equal to the uncached model column and jac, the cached entries copied.
    S = 1 under the cosine: d cos / d x is identically 0 (cos = +-1 for any x) while its two terms u / den and m v / |v|^2 are of size
    1 / |x|; both sides hold rounding residue, so jac is compared on the scale of those terms there (same 1e-5)."""
    h = _h()
    for n_rest in C.MATRIX_NREST:
        ref, x0, rest = C.matrix_inputs(S, mode, n_rest)
        for lt in (1, 2, 3):
            for ideal in (False, True):
                what = f"S{S}-mode{mode}-lt{lt}-nr{n_rest}-ideal{int(ideal)}"
                m64, j64 = C.matrix_oracle(ref, x0, rest, mode, lt, ideal, torch.float64)
                m32, j32 = C.matrix_oracle(ref, x0, rest, mode, lt, ideal, torch.float32)
                mat, jac = matrix_launch(ref, x0, rest, mode, lt, ideal, "fwd", dev)
                rows, jac_r = matrix_launch(ref, x0, rest, mode, lt, ideal, "rows", dev)
                assert torch.equal(rows[:, :-1], mat) and torch.equal(jac_r, jac) and bool((rows[:, -1] == 1.0).all()), what
                gate(f"risk_matrix.mode{mode}.lt{lt}.mat", mat, m64, m32, what)
                if S == 1 and lt == 2 and mode == 1:
                    assert float((jac.cpu().double() * x0.double().abs()).abs().max()) <= TOL, what
                else:
                    gate(f"risk_matrix.mode{mode}.lt{lt}.jac", jac, j64, j32, what)
                if mode != 1 and not ideal and n_rest:
                    stride = n_rest + 2
                    cache = torch.full((C.MATRIX_B, stride), -7.0, dtype=torch.float32, device=dev)
                    cache[:, :n_rest] = mat[:, 1:]
                    cm = torch.full((C.MATRIX_B, 1 + n_rest), NAN, dtype=torch.float32, device=dev)
                    cj = torch.full((C.MATRIX_B, S), NAN, dtype=torch.float32, device=dev)
                    rd, xd = ref.to(dev), x0.to(dev)                     # named: the launch reads them after this line
                    _check(h.ltr_risk_matrix_cached_fwd(_p(rd), _p(xd), _p(cache), stride, C.MATRIX_B, S, n_rest, mode, lt,
                                                        _p(cm), _p(cj), _stream()), "ltr_risk_matrix_cached_fwd")
                    assert torch.equal(cm, mat) and torch.equal(cj, jac), what


@pytest.mark.parametrize("big", [80.0, 100.0])
@pytest.mark.parametrize("S", [3, 257, 2048])
def test_matrix_softmax_stays_finite_with_huge_scores(S, big, dev):
    """Scores of +-80 (and +-100, where expf itself overflows fp32): the slate softmax subtracts the maximum, so the matrix stays
    finite and equals the fp64 oracle where a naive exponent would give inf / inf."""
    gen = torch.Generator().manual_seed(77 + S)
    ref = torch.randint(0, 5, (C.MATRIX_B, S), generator=gen).float()
    x0 = torch.where(torch.rand(C.MATRIX_B, S, generator=gen) < 0.5, torch.tensor(big), torch.tensor(-big))
    x0[0, 0], x0[1, S - 1], x0[2, S // 2] = big, big, big
    rest = x0.flip(1)[:, :, None].contiguous() + torch.randn(C.MATRIX_B, S, 1, generator=gen)
    for mode in (0, 2):
        for lt in (1, 2, 3):
            what = f"S{S}-big{big:g}-mode{mode}-lt{lt}"
            m64, j64 = C.matrix_oracle(ref, x0, rest, mode, lt, True, torch.float64)
            m32, j32 = C.matrix_oracle(ref, x0, rest, mode, lt, True, torch.float32)
            mat, jac = matrix_launch(ref, x0, rest, mode, lt, True, "fwd", dev)
            assert bool(torch.isfinite(mat).all()) and bool(torch.isfinite(jac).all()), what
            gate(f"risk_matrix.huge_scores.mode{mode}.lt{lt}.mat", mat, m64, m32, what)
            gate(f"risk_matrix.huge_scores.mode{mode}.lt{lt}.jac", jac, j64, j32, what)


def test_scores_grad_beyond_its_grid_cap(dev):
    """ltr_risk_scores_grad at B = 4100, S = 257 (more than 4096 x 256 elements: the grid-stride loop runs), dmat read in place at a
    row stride of 5: exactly jac * dmat[:, :1] (one fp32 multiplication per element on both sides)."""
    B, S = 4100, 257
    gen = torch.Generator().manual_seed(41)
    jac = torch.randn(B, S, generator=gen).to(dev)
    dmat = torch.randn(B, 5, generator=gen).to(dev)
    ds = torch.full((B, S), NAN, dtype=torch.float32, device=dev)
    _check(_h().ltr_risk_scores_grad(_p(jac), _p(dmat), 5, B, S, _p(ds), _stream()), "ltr_risk_scores_grad")
    assert torch.equal(ds, jac * dmat[:, :1])
