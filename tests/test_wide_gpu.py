"""GPU: FC scorers wider than 136 features (csrc/ltr_wide.hip, ltr_mi355x.wide) -- the exact-fp32 GEMM elementwise against fp64 at a
derived bound, its epilogues bitwise from its own raw output, and WideFusedRanker's steps (rectangular, ragged, risk, deferred
normalisation, dropout stream) against the fp64 oracles at the project's bars: 1e-5 on losses and scores, assert_grads on gradients."""
import struct

import numpy as np
import pytest
import torch

import ragged_cases as RC
import wide_cases as WC
from conftest import ledger_record
from conftest import relerr as _relerr
from test_ragged_gpu import _oracle_ragged_step
from test_risk_fused_gpu import _assert_grads as risk_assert_grads
from test_risk_fused_gpu import _assert_loss as risk_assert_loss
from test_risk_fused_gpu import _data as risk_data
from test_risk_fused_gpu import _oracle as risk_oracle
from test_scorer_gpu import _make, _oracle_step, assert_grads

pytestmark = pytest.mark.gpu
TOL = 1e-5
LAMBDA = dict(weighing_scheme="ndcgLoss2PP_scheme", reduction="sum")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    return torch.device("cuda:0")


def relerr(a, b, quantity):
    e = _relerr(a, b)
    print(f"{quantity}: rel err {e:.3e}")
    ledger_record(quantity, e)
    return e


# ---------------------------------------------------------------------------------------------------------------- ltr_gemm_f32
def _store(rng, shape, off, dev):
    """A random fp32 [rows][ld] operand whose base is `off` floats past a 16-byte boundary -> (device view, host array)."""
    host = rng.standard_normal(shape).astype(np.float32)
    buf = torch.empty(host.size + 4, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + host.size].view(*shape)
    view.copy_(torch.from_numpy(host))
    return view, host


def _sum_partials(parts, nsplit, n, dev):
    from ltr_mi355x._lib import check, lib
    out = torch.empty(n, dtype=torch.float32, device=dev)
    check(lib().ltr_enc_sum_partials(parts.data_ptr(), nsplit, n, 0, out.data_ptr(), torch.cuda.current_stream().cuda_stream),
          "ltr_enc_sum_partials")
    return out


@pytest.mark.parametrize("c", WC.gemm_cases(), ids=WC.case_id)
def test_gemm_elementwise_vs_fp64(c, dev):
    from ltr_mi355x.wide import gemm_f32
    M, N, K, S = c["M"], c["N"], c["K"], c["splits"]
    rng = np.random.default_rng(1000 * M + 10 * N + K + S)
    (ar, lda), (br, ldb) = WC.operand_shapes(c)
    a_dev, a_host = _store(rng, (ar, lda), c["off_a"], dev)
    b_dev, b_host = _store(rng, (br, ldb), c["off_b"], dev)
    ak, bk = WC.FORMS[c["form"]]
    vec_a, vec_b = a_dev.data_ptr() % 16 == 0 and lda % 4 == 0, b_dev.data_ptr() % 16 == 0 and ldb % 4 == 0
    print(f"{WC.case_id(c)}: A {'16' if vec_a else '4'}-byte loads, B {'16' if vec_b else '4'}-byte loads")
    A, B = WC.logical(c, a_host, b_host)
    bias = rng.standard_normal(N).astype(np.float32) if S == 1 else None
    ref = A.astype(np.float64) @ B.astype(np.float64).T + (0.0 if bias is None else bias.astype(np.float64)[None, :])
    ldc = N + (3 if M % 2 else 0)                       # a padded output row now and then
    out = torch.full((S, M, ldc), float("nan"), dtype=torch.float32, device=dev)
    gemm_f32(a_dev, b_dev, out, M, N, K, lda, ldb, ldc, a_kmajor=ak, b_kmajor=bk, splits=S,
             bias=None if bias is None else torch.from_numpy(bias).to(dev))
    if S > 1:
        got = _sum_partials(out, S, M * ldc, dev).view(M, ldc)
        # every slice wrote all of its M x N block (a slice without k: zeros), and nothing else
        assert not torch.isnan(out[:, :, :N]).any()
    else:
        got = out[0]
    assert torch.isnan(out[:, :, N:]).all()
    got = got[:, :N].cpu().numpy().astype(np.float64)
    bound = WC.gemm_bound(A, B, bias)
    worst = float((np.abs(got - ref) / np.maximum(bound, 1e-300)).max())
    print(f"{WC.case_id(c)}: worst |C - C64| / bound = {worst:.3f}")
    ledger_record("ltr_gemm_f32 max|C - C64| / ((K + 4) 2^-24 (|A||B|^T + |bias|))", worst, tol=1.0)
    assert worst <= 1.0


def test_gemm_cases_cover_both_load_paths_per_operand():
    """Host arithmetic only (the rule of include/ltr_mi355x.h on the case list), kept next to the cases it vouches for."""
    seen = set()
    for c in WC.gemm_cases():
        (_, lda), (_, ldb) = WC.operand_shapes(c)
        for name, ld, off, km in (("A", lda, c["off_a"], WC.FORMS[c["form"]][0]), ("B", ldb, c["off_b"], WC.FORMS[c["form"]][1])):
            seen.add((name, km, ld % 4 == 0 and off == 0))
    assert seen == {(n, km, v) for n in "AB" for km in (0, 1) for v in (False, True)}


def _p_eff(p):
    """The probability a drop code carries: float32(p) with its lowest bit cleared (ltr_mi355x.scorer.drop_code)."""
    from ltr_mi355x.scorer import drop_code
    code = drop_code(True, p)
    return np.float32(0.5) if code == 1 else np.float32(struct.unpack("<f", struct.pack("<I", code & ~1))[0])


def test_gemm_epilogues_from_the_raw_output(dev):
    from ltr_mi355x.scorer import drop_code, dropout_keep_mask
    from ltr_mi355x.wide import ACT_RELU, ACT_SIGMOID, GATE_RELU, GATE_SIGMOID, gemm_f32
    M, N, K = 70, 137, 33
    rng = np.random.default_rng(5)
    a, ah = _store(rng, (M, K), 0, dev)
    b, bh = _store(rng, (N, K), 0, dev)
    bias_h = rng.standard_normal(N).astype(np.float32)
    bias = torch.from_numpy(bias_h).to(dev)

    def run(**kw):
        out = torch.empty((M, N), dtype=torch.float32, device=dev)
        gemm_f32(a, b, out, M, N, K, K, K, N, **kw)
        return out.cpu().numpy()

    raw = run()
    assert np.array_equal(run(), raw)                                   # same inputs, same bits
    rb = run(bias=bias)
    assert np.array_equal(rb, raw + bias_h[None, :])
    assert np.array_equal(run(bias=bias, act=ACT_RELU), np.maximum(rb, np.float32(0)))
    sg = run(bias=bias, act=ACT_SIGMOID)
    assert relerr(sg, 1.0 / (1.0 + np.exp(-rb.astype(np.float64))), "ltr_gemm_f32 sigmoid epilogue") < TOL
    # gates through a saved post-activation tensor
    gate_h = np.maximum(rng.standard_normal((M, N)), 0).astype(np.float32)
    gate = torch.from_numpy(gate_h).to(dev)
    for scale in (np.float32(1.0), np.float32(1) / (np.float32(1) - np.float32(0.3))):
        got = run(gate=gate, ldg=N, gate_kind=GATE_RELU, gate_scale=float(scale))
        assert np.array_equal(got, np.where(gate_h > 0, raw * scale, np.float32(0)))
    sig_h = rng.uniform(0, 1, (M, N)).astype(np.float32)
    got = run(gate=torch.from_numpy(sig_h).to(dev), ldg=N, gate_kind=GATE_SIGMOID)
    assert np.array_equal(got, raw * (sig_h * (np.float32(1) - sig_h)))
    # dropout: the scorers' keep stream, as ltr_dropout_keep_mask[_p] exports it, and explicit masks
    seed = 0x1234_5678_9ABC_DEF0
    for p in (0.5, 0.3):
        scale = np.float32(1) / (np.float32(1) - _p_eff(p))
        for layer in (0, 1):
            keep = dropout_keep_mask(seed, layer, M, N, dev, p).cpu().numpy()
            assert 0.5 * (1 - p) < keep.mean() < 1 - 0.5 * p
            got = run(dropout=drop_code(True, p), drop_layer=layer, seed=seed)
            assert np.array_equal(got, np.where(keep != 0, raw * scale, np.float32(0))), (p, layer)
        mask_h = (rng.uniform(size=(M, N)) < 0.6).astype(np.uint8)
        got = run(dropout=drop_code(True, p), keep=torch.from_numpy(mask_h).to(dev), seed=seed)
        assert np.array_equal(got, np.where(mask_h != 0, raw * scale, np.float32(0)))
    # the whole forward epilogue in its order: bias, ReLU, dropout
    keep = dropout_keep_mask(seed, 0, M, N, dev, 0.5).cpu().numpy()
    got = run(bias=bias, act=ACT_RELU, dropout=1, drop_layer=0, seed=seed)
    assert np.array_equal(got, np.where(keep != 0, np.maximum(rb, np.float32(0)) * np.float32(2), np.float32(0)))


@pytest.mark.parametrize("T,N,pad,nblk", [(1, 1, 0, 4), (185, 137, 0, 7), (300, 64, 3, 512), (257, 1024, 0, 3), (70, 65, 0, 1)])
def test_colsum_vs_fp64(T, N, pad, nblk, dev):
    """|sum - sum64| <= (T + 5) 2^-24 sum |w y|: T - 1 additions in any order, the product with the row weight, the fp64 -> fp32 store."""
    from ltr_mi355x._lib import check, lib
    rng = np.random.default_rng(T + N)
    y, yh = _store(rng, (T, N + pad), 0, dev)
    w, wh = _store(rng, (T,), 0, dev)
    for wt, wth in ((None, np.ones(T)), (w, wh.astype(np.float64))):
        parts = torch.full((nblk, N), float("nan"), dtype=torch.float32, device=dev)
        check(lib().ltr_colsum_f32(y.data_ptr(), T, N, N + pad, None if wt is None else wt.data_ptr(), parts.data_ptr(), nblk,
                                   torch.cuda.current_stream().cuda_stream), "ltr_colsum_f32")
        got = _sum_partials(parts, nblk, N, dev).cpu().numpy().astype(np.float64)
        prod = yh[:, :N].astype(np.float64) * wth[:, None]
        bound = (T + 5) * 2.0 ** -24 * np.abs(prod).sum(axis=0)
        assert (np.abs(got - prod.sum(axis=0)) <= bound).all()


# ---------------------------------------------------------------------------------------------------------------- the step
def _grads(net):
    return {k: p.grad.detach().cpu().numpy() for k, p in net.named_parameters()}


def _batch(F, B, S, loss, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, F, generator=g)
    y = torch.randint(0, 5, (B, S), generator=g).float()
    if loss != "listnet":
        y[1 % B, -5:] = -1.0                           # one slate with trailing padding, for the two masking losses
    return x, y, g


def _step_case(kind, F, loss, B, S, dev, red="sum"):
    from ltr_mi355x.wide import WideFusedRanker
    k = "triple" if kind == "triple" else "double"
    net, sd = _make(k, dev, F, F=F)
    net.train(kind == "double_train")
    x, y, g = _batch(F, B, S, loss, F)
    k1 = k2 = None
    if kind == "double_train":
        k1 = (torch.rand(B, S, F, generator=g) < 0.5).float()
        k2 = (torch.rand(B, S, F, generator=g) < 0.5).float()
    kw = dict(LAMBDA, k=None, sigma=1.0, mu=10.0, reduction=red, reduction_log="binary")
    rl, rg, _ = _oracle_step(k, sd, x, y, loss, k1, k2, lambda_kw=kw)
    _, rg32, _ = _oracle_step(k, sd, x, y, loss, k1, k2, dtype=torch.float32, lambda_kw=kw)
    extra = dict(LAMBDA, reduction=red) if loss == "lambdaLoss" else {}
    ranker = WideFusedRanker(net, loss=loss, **extra)
    out = ranker.step(x.to(dev), y.to(dev), keep1=None if k1 is None else k1.to(dev), keep2=None if k2 is None else k2.to(dev))
    assert relerr(out.cpu().numpy(), rl, f"wide step {loss} loss") < TOL
    assert_grads(_grads(net), rg, ref32=rg32)
    flat = torch.cat([p.grad.reshape(-1) for p in net.parameters()])
    assert torch.equal(flat, ranker.flat_grad)         # p.grad aliases the flat buffer, in parameters() order
    return ranker


@pytest.mark.parametrize("loss", ["approxNDCG", "listnet", "lambdaLoss"])
@pytest.mark.parametrize("F", [137, 220, 519])
@pytest.mark.parametrize("kind", ["double_eval", "double_train", "triple"])
def test_step_vs_oracle(kind, F, loss, dev):
    _step_case(kind, F, loss, 5, 37, dev)               # 185 documents: a multiple of no tile


@pytest.mark.parametrize("kind", ["double_train", "triple"])
def test_step_at_the_widest_network(kind, dev):
    _step_case(kind, 1024, "approxNDCG", 5, 37, dev)


def test_step_multi_tile_multi_split(dev):
    r = _step_case("double_train", 220, "approxNDCG", 37, 128, dev)        # 4 736 documents: 74 row tiles, dW split over the documents
    assert WC.splits(220, 220, 37 * 128, r.grid) > 1


def test_step_lambda_mean(dev):
    _step_case("double_eval", 220, "lambdaLoss", 5, 37, dev, red="mean")


def test_scores_vs_oracle_and_zero_size_backward(dev):
    """The forward launcher's scores on their own (the step only shows them through the loss), and the backward's zero-size call."""
    import ctypes
    from ltr_mi355x._lib import check, lib
    from ltr_mi355x.scorer import triple_fold
    h, st = lib(), torch.cuda.current_stream().cuda_stream
    F, n = 220, 185
    for kind in ("double", "triple"):
        net, sd = _make(kind, dev, F, F=F)
        x = torch.randn(n, F, generator=torch.Generator().manual_seed(3))
        rs = _oracle_step(kind, sd, x[None], torch.zeros(1, n), "listnet")[2]
        ps = [p.detach() for p in net._ltr_params()]
        code, H1, H2 = 0, F, F
        if kind == "triple":
            ps, code, H1, H2 = triple_fold(ps, 1) + [ps[5]], 1, 32, 32
        ptrs = (ctypes.c_void_p * len(ps))(*[t.data_ptr() for t in ps])
        X = x.to(dev)
        scores = torch.empty(n, device=dev)
        acts = torch.empty(h.ltr_wide_acts_floats(code, F, H1, H2, n), device=dev)
        check(h.ltr_wide_forward_save(code, F, H1, H2, X.data_ptr(), n, ptrs, 0, 0, None, None, scores.data_ptr(), acts.data_ptr(), st),
              "ltr_wide_forward_save")
        assert relerr(scores.cpu().numpy(), rs.reshape(-1), f"wide forward scores ({kind})") < TOL
        n_par = H1 * F + H1 + (H2 * H1 + H2 if code == 0 else 0) + (H2 if code == 0 else H1) + 1
        flat = torch.full((n_par + 1,), 7.0, device=dev)
        ws = torch.empty(16, device=dev)
        check(h.ltr_wide_backward_saved(code, F, H1, H2, X.data_ptr(), 0, ptrs, 0, acts.data_ptr(), scores.data_ptr(), ws.data_ptr(), 8,
                                        flat.data_ptr(), st), "ltr_wide_backward_saved")
        assert float(flat[:n_par].abs().max()) == 0.0 and float(flat[n_par]) == 7.0


# ---------------------------------------------------------------------------------------------------------------- dropout stream
@pytest.mark.parametrize("p", [0.5, 0.3])
def test_seeded_dropout_is_the_exported_stream(p, dev):
    from ltr_mi355x.scorer import dropout_keep_mask
    from ltr_mi355x.wide import WideFusedRanker
    F, B, S = 220, 5, 37
    net, _ = _make("double", dev, 11, F=F)
    net.train()
    net.dropout.p = p
    x, y, _ = _batch(F, B, S, "approxNDCG", 12)
    X, Y = x.to(dev), y.to(dev)
    ranker = WideFusedRanker(net, loss="approxNDCG")
    seed = 0xFEDC_BA98_7654_3210
    ranker.step(X, Y, seed=seed)
    a = ranker.flat.clone()
    assert torch.isfinite(a).all() and float(ranker.flat_grad.abs().max()) > 0.0
    ranker.step(X, Y, seed=seed)
    assert torch.equal(a, ranker.flat)                                  # the same seed: the same bits
    ranker.step(X, Y, keep1=dropout_keep_mask(seed, 0, B * S, F, dev, p), keep2=dropout_keep_mask(seed, 1, B * S, F, dev, p))
    assert torch.equal(a, ranker.flat)                                  # the exported masks replayed: the same bits
    ranker.step(X, Y)
    b = ranker.flat.clone()
    ranker.step(X, Y)
    assert not torch.equal(b, ranker.flat) and not torch.equal(a, b)    # the default seed moves with every step


# ---------------------------------------------------------------------------------------------------------------- ragged
def _slates(lengths, dev):
    from ltr_mi355x.ragged import RaggedSlates
    return RaggedSlates(RC.bounds_of(lengths), device=dev)


@pytest.mark.parametrize("loss,red", [("approxNDCG", "sum"), ("listnet", "sum"), ("lambdaLoss", "sum"), ("lambdaLoss", "mean")])
@pytest.mark.parametrize("kind", ["double_train", "triple"])
def test_equal_lengths_are_the_rectangular_step_bits(kind, loss, red, dev):
    from ltr_mi355x.wide import WideFusedRanker
    Q, S, F = 5, 37, 220
    net, _ = _make("triple" if kind == "triple" else "double", dev, 31, F=F)
    net.train(kind == "double_train")
    ranker = WideFusedRanker(net, loss=loss, **(dict(LAMBDA, reduction=red) if loss == "lambdaLoss" else {}))
    g = torch.Generator().manual_seed(737)
    X, Y = torch.randn(Q * S, F, generator=g).to(dev), torch.randint(0, 5, (Q * S,), generator=g).float().to(dev)
    kw = dict(seed=4321) if kind == "double_train" else {}
    ranker.step(X.view(Q, S, F), Y.view(Q, S), **kw)
    a = ranker.flat_ext.clone()
    assert torch.isfinite(a).all() and float(ranker.flat_grad.abs().max()) > 0.0
    ranker.flat_ext.zero_()
    ranker.step_ragged(X, Y, _slates([S] * Q, dev), **kw)
    assert torch.equal(a, ranker.flat_ext)


RAGGED_LENGTHS = [1, 2, 37, 64, 65, 130, 300]


@pytest.mark.parametrize("loss", ["approxNDCG", "listnet", "lambdaLoss"])
@pytest.mark.parametrize("kind", ["double_train", "triple"])
def test_step_ragged_vs_per_query_oracle(kind, loss, dev):
    from ltr_mi355x.wide import WideFusedRanker
    F = 220
    k = "triple" if kind == "triple" else "double"
    net, sd = _make(k, dev, 31, F=F)
    net.train(kind == "double_train")
    ranker = WideFusedRanker(net, loss=loss, **(LAMBDA if loss == "lambdaLoss" else {}))
    bounds, n = RC.bounds_of(RAGGED_LENGTHS), sum(RAGGED_LENGTHS)
    # lambdaLoss weights every pair by the RANKS of the predicted scores (lambdaL.py:36-60): two documents of one query whose exact
    # scores differ by less than fp32 resolves rank either way in any fp32 implementation, and one swapped pair moves the loss by
    # ~5e-4 (seed 5 holds a pair 1.3e-8 apart at |score| ~ 0.3 for the TripleLayerNet; tests/test_scorer_gpu.py::
    # test_slate512_lambda_through_modules meets the same).  Take the first seed whose fp64 ORACLE scores have no such tie.
    for data_seed in range(5, 64):
        g = torch.Generator().manual_seed(data_seed)
        x, y = torch.randn(n, F, generator=g), torch.randint(0, 5, (n,), generator=g).float()
        k1 = k2 = None
        if kind == "double_train":
            k1, k2 = (torch.rand(n, F, generator=g) < 0.5).float(), (torch.rand(n, F, generator=g) < 0.5).float()
        so = _oracle_step(k, sd, x[None], y[None], "listnet", None if k1 is None else k1[None], None if k2 is None else k2[None])[2][0]
        if min(float(np.diff(np.sort(so[a:b])).min()) for a, b in zip(bounds[:-1], bounds[1:]) if b - a > 1) > 4e-7:
            break                                        # 4 x the kernels' score error (~1e-7)
    else:
        raise AssertionError("no tie-free seed")
    rl, rg = _oracle_ragged_step(k, sd, x, y, bounds, loss, "sum", k1, k2)
    _, rg32 = _oracle_ragged_step(k, sd, x, y, bounds, loss, "sum", k1, k2, dtype=torch.float32)
    kw = {} if k1 is None else dict(keep1=k1.to(dev), keep2=k2.to(dev))
    out = ranker.step_ragged(x.to(dev), y.to(dev), _slates(RAGGED_LENGTHS, dev), **kw)
    assert relerr(out.cpu().numpy(), rl, f"wide step_ragged {loss} loss") < TOL
    assert_grads(_grads(net), rg, ref32=rg32)


# ---------------------------------------------------------------------------------------------------------------- risk losses
@pytest.mark.parametrize("name", ["geoRiskListnetLoss", "tRiskLambdaLoss"])
@pytest.mark.parametrize("kind", ["double_train", "triple"])
def test_risk_step_vs_oracle(kind, name, dev):
    from ltr_mi355x.wide import WideFusedRanker
    F, B, S = 220, 5, 37
    k = "triple" if kind == "triple" else "double"
    net, sd = _make(k, dev, 3, F=F)
    net.train(kind == "double_train")
    x, y, yb = risk_data(name, B, S, F, seed=100 * S + B)
    keep, kw = None, {}
    if kind == "double_train":
        g = torch.Generator().manual_seed(7 + S)
        keep = ((torch.rand(B, S, F, generator=g) < 0.5).float(), (torch.rand(B, S, F, generator=g) < 0.5).float())
        kw = dict(keep1=keep[0].to(dev), keep2=keep[1].to(dev))
    ranker = WideFusedRanker(net, loss=name)
    out = float(ranker.step(x.to(dev), y.to(dev), y_base=yb.to(dev), **kw))
    args = dict(ranker.risk.args)
    rl, rg = risk_oracle(name, k, sd, x, y, yb, args, keep)
    rl32, rg32 = risk_oracle(name, k, sd, x, y, yb, args, keep, dtype=torch.float32)
    risk_assert_loss(name, out, rl, rl32)
    risk_assert_grads(name, _grads(net), rg, rg32)


def test_risk_step_cached_columns_are_the_same_bits(dev):
    from ltr_mi355x.wide import WideFusedRanker
    F, B, S = 220, 5, 37
    name = "geoRiskListnetLoss"
    net, _ = _make("double", dev, 3, F=F)
    net.train()
    x, y, yb = risk_data(name, B, S, F, seed=9)
    X, Y, YB = x.to(dev), y.to(dev), yb.to(dev)
    ranker = WideFusedRanker(net, loss=name)
    ranker.step(X, Y, y_base=YB, seed=77)
    a = ranker.flat.clone()
    assert torch.isfinite(a).all() and float(ranker.flat_grad.abs().max()) > 0.0
    ranker.flat.zero_()
    ranker.step(X, Y, base_cols=ranker.baseline_columns(Y, YB), seed=77)
    assert torch.equal(a, ranker.flat)


# ---------------------------------------------------------------------------------------------------------------- deferred normalisation
@pytest.mark.parametrize("loss,red", [("approxNDCG", "sum"), ("lambdaLoss", "mean")])
def test_two_half_batches_with_deferred_normalisation(loss, red, dev):
    """What QueryShardedTrainer does with two ranks, in one process: sum-form halves, `flat_ext` added, one division."""
    from ltr_mi355x.wide import WideFusedRanker
    F, B, S = 220, 6, 37
    net, _ = _make("double", dev, 13, F=F)
    net.eval()
    x, y, _ = _batch(F, B, S, loss, 14)
    X, Y = x.to(dev), y.to(dev)
    ranker = WideFusedRanker(net, loss=loss, **(dict(LAMBDA, reduction=red) if loss == "lambdaLoss" else {}))
    ranker.step(X, Y)
    full = ranker.flat.clone()
    ranker.step(X[:3], Y[:3], defer_norm=True)
    half = ranker.flat_ext.clone()
    ranker.step(X[3:], Y[3:], defer_norm=True)
    ranker.flat_ext.add_(half)
    ranker.finish_norm()
    assert relerr(ranker.flat.cpu().numpy(), full.cpu().numpy(), f"wide deferred normalisation ({loss})") < 1e-6
