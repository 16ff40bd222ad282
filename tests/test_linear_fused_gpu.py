"""GPU: the fused training step of FC-only make_model rankers (csrc/ltr_linear.hip, ltr_mi355x/linear.py).

FCModel / OutputLayer hard-wire Identity activations (multiLayer.py:29, :105), so with no active dropout the network folds into one
scoring vector.  Checked against a fp64 layer-by-layer oracle (tests/test_linear_fused_cpu.py) plus oracle/'s losses: loss 1e-5
relative, gradients at the fused DoubleLayerNet tests' bar (test_scorer_gpu.assert_grads):
  * ltr_linear_fold / ltr_linear_unfold_grads against the chain rule in fp64 (0, 1, 3, 4 layers; input_norm; F 8 .. 1024);
  * FusedRanker(make_model(config.json "model")) for the three losses, one-launch and multi-launch slates, ragged / padded
    batches, lambdaLoss mean and k, apply_sigmoid, input_norm, and the r6 reference goldens;
  * determinism, 20 Adam steps, dropout / encoder / d_output rules, the precision gain over the module path, two ranks."""
import copy
import ctypes
import os
import socket
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ledger_record
from test_linear_fused_cpu import golden_r6, linear_forward, oracle_step
from test_scorer_gpu import assert_grads

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIG = {"fc_model": {"sizes": [128, 256, 128], "input_norm": False, "activation": None, "dropout": 0.0}, "transformer": False,
          "post_model": {"output_activation": "Sigmoid", "d_output": 1}}      # config.json "model"
SIZES = [128, 256, 128]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    return torch.device("cuda:0")


def _model(dev, seed=5, F=136, sizes=SIZES, input_norm=False, dropout=0.0):
    from architeture.multiLayer import make_model
    torch.manual_seed(seed)
    m = make_model(dict(sizes=list(sizes), input_norm=input_norm, activation=None, dropout=dropout), False,
                   dict(output_activation="Sigmoid", d_output=1), F)
    if input_norm:                                   # non-trivial gamma / beta
        with torch.no_grad():
            m.input_layer.input_norm.weight.uniform_(0.5, 1.5)
            m.input_layer.input_norm.bias.uniform_(-0.2, 0.2)
    return m.to(dev)


def _data(B, S, F=136, seed=0, pad=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, F, generator=g)
    y = torch.randint(0, 5, (B, S), generator=g).float()
    if pad:
        y[-1, -pad:] = -1.0
    return x, y


def _as_dict(grads):
    return {str(i): np.asarray(g) for i, g in enumerate(grads)}


def _check(net, ranker, x, y, loss, dev, sizes=SIZES, input_norm=False, lambda_kw=None, apply_sigmoid=False, **step_kw):
    l = ranker.step(x.to(dev), y.to(dev), **step_kw)
    torch.cuda.synchronize()
    params = net._ltr_params()
    got = [p.grad.detach().cpu().numpy() for p in params]
    lr, gr = oracle_step(params, x, y, sizes, input_norm, loss, lambda_kw=lambda_kw, apply_sigmoid=apply_sigmoid)
    e = abs(float(l) - lr) / max(abs(lr), 1e-30)
    ledger_record("loss", e)
    assert e <= 1e-5, (float(l), lr)
    top = max(float(np.abs(g).max()) for g in gr)
    if top < 1e-12:                                  # single-document slates: the loss is constant, every gradient exactly 0
        assert max(float(np.abs(g).max()) for g in got) < 1e-6
    else:
        # long slates: d loss / d s comes from the fp32 loss kernels, whose own rounding the fp32 oracle measures (the fused
        # DoubleLayerNet tests' relaxed bar, max(1e-5, 4 x that noise))
        ref32 = None
        if x.shape[1] >= 1000:
            ref32 = _as_dict(oracle_step(params, x, y, sizes, input_norm, loss, dtype=torch.float32, lambda_kw=lambda_kw,
                                         apply_sigmoid=apply_sigmoid)[1])
        assert_grads(_as_dict(got), _as_dict(gr), ref32=ref32)
    return float(l), got


# ------------------------------------------------------------------------------------------------------ fold / unfold kernels
def _rand_params(F, sizes, input_norm, seed):
    g = torch.Generator().manual_seed(seed)
    ps = []
    if input_norm:
        ps += [torch.rand(F, generator=g) + 0.5, torch.randn(F, generator=g) * 0.1]
    n = F
    for w in sizes:
        ps += [torch.randn(w, n, generator=g) / n ** 0.5, torch.randn(w, generator=g) * 0.1]
        n = w
    return ps + [torch.randn(1, n, generator=g) / n ** 0.5, torch.randn(1, generator=g)]


def _chain64(ps, F, sizes, input_norm):
    p = [t.double() for t in ps]
    i = 2 if input_norm else 0
    Ws = [p[i + 2 * k] for k in range(len(sizes))]
    bs = [p[i + 2 * k + 1] for k in range(len(sizes))]
    wo, bo = p[-2][0], p[-1]
    v = [None] * (len(sizes) + 1)
    v[-1] = wo
    for k in range(len(sizes), 0, -1):
        v[k - 1] = v[k] @ Ws[k - 1]
    beff = bo[0] + sum(float(v[k + 1] @ bs[k]) for k in range(len(sizes)))
    return p, Ws, bs, v, beff


@pytest.mark.parametrize("F", [8, 64, 136, 1024])
@pytest.mark.parametrize("input_norm", [False, True])
@pytest.mark.parametrize("L", [0, 1, 3, 4])
def test_fold_unfold_kernels(dev, F, input_norm, L):
    from ltr_mi355x import lib
    from ltr_mi355x.functional import _stream
    sizes = [64, 96, 32, 48][:L]
    ps = [t.to(dev).contiguous() for t in _rand_params(F, sizes, input_norm, 10 * L + F)]
    h = lib()
    cs = (ctypes.c_int * max(1, L))(*sizes)
    ptrs = (ctypes.c_void_p * len(ps))(*[t.data_ptr() for t in ps])
    ws = torch.empty(int(h.ltr_linear_ws_doubles(L, F, cs)), dtype=torch.float64, device=dev)
    weff = torch.empty(F + 2, dtype=torch.float32, device=dev)
    assert h.ltr_linear_fold(L, F, cs, int(input_norm), ptrs, ws.data_ptr(), weff.data_ptr(), _stream()) == 0
    p, Ws, bs, v, beff = _chain64([t.cpu() for t in ps], F, sizes, input_norm)
    w = v[0]
    c = beff
    if input_norm:
        c += float(v[0] @ p[1])
        w = v[0] * p[0]
    got = weff.cpu().double()
    assert float((got[:F] - w).abs().max()) <= 1e-6 * float(w.abs().max())
    assert abs(float(got[F]) - c) <= 1e-6 * max(1.0, abs(c))
    # unfold on random partials [grid][F + 1]
    grid = 3
    part = torch.randn(grid, F + 1, generator=torch.Generator().manual_seed(F + L)).to(dev)
    flat = torch.full((sum(t.numel() for t in ps),), float("nan"), dtype=torch.float32, device=dev)
    assert h.ltr_linear_unfold_grads(L, F, cs, int(input_norm), ptrs, part.data_ptr(), grid, ws.data_ptr(), flat.data_ptr(), _stream()) == 0
    pd = part.cpu().double()
    Gh, G1 = pd[:, :F].sum(0), float(pd[:, F].sum())
    want = []
    H = Gh
    if input_norm:
        want += [v[0] * Gh, v[0] * G1]
        H = p[0] * Gh + p[1] * G1
    for k in range(L):
        want += [torch.outer(v[k + 1], H), v[k + 1] * G1]
        H = Ws[k] @ H + bs[k] * G1
    want += [H.reshape(1, -1), torch.tensor([G1], dtype=torch.float64)]
    want = torch.cat([t.reshape(-1) for t in want])
    got = flat.cpu().double()
    assert not torch.isnan(got).any()
    assert float((got - want).abs().max()) <= 1e-6 * float(want.abs().max())


# ------------------------------------------------------------------------------------------------------ FusedRanker(make_model)
@pytest.mark.parametrize("loss", ["approxNDCG", "listnet", "lambdaLoss"])
@pytest.mark.parametrize("S,B", [(32, 37), (64, 5), (128, 9), (1, 6), (7, 5), (100, 7), (250, 3), (1000, 2), (2048, 2)])
def test_config_network_vs_fp64(dev, loss, S, B):
    net = _model(dev)
    from ltr_mi355x.scorer import FusedRanker
    kw = dict(weighing_scheme="ndcgLoss2PP_scheme") if loss == "lambdaLoss" else {}
    r = FusedRanker(net, loss=loss, **kw)
    assert type(r).__name__ == "LinearFusedRanker"
    x, y = _data(B, S, seed=S + B, pad=min(3, S - 1))
    _check(net, r, x, y, loss, dev, lambda_kw=kw or None)
    for p, gv in zip(r.params, r._grad_views):
        assert p.grad is gv


@pytest.mark.parametrize("S", [64, 100])
@pytest.mark.parametrize("loss", ["approxNDCG", "listnet", "lambdaLoss"])
def test_input_norm_network(dev, S, loss):
    net = _model(dev, seed=8, F=64, sizes=[32, 16], input_norm=True)
    from ltr_mi355x.scorer import FusedRanker
    kw = dict(weighing_scheme="ndcgLoss2PP_scheme") if loss == "lambdaLoss" else {}
    r = FusedRanker(net, loss=loss, **kw)
    x, y = _data(6, S, F=64, seed=3)
    x = x * 3.0 + 1.5                                # rows with a mean and a spread for the LayerNorm
    _check(net, r, x, y, loss, dev, sizes=[32, 16], input_norm=True, lambda_kw=kw or None)


@pytest.mark.parametrize("S", [32, 128, 100])
@pytest.mark.parametrize("kw", [dict(reduction="mean"), dict(k=5), dict(k=3, reduction="mean", weighing_scheme="lamdbaRank_scheme"),
                                dict(weighing_scheme="rankNet_scheme", sigma=2.0)])
def test_lambda_variants(dev, S, kw):
    net = _model(dev, seed=9)
    from ltr_mi355x.scorer import FusedRanker
    r = FusedRanker(net, loss="lambdaLoss", **kw)
    x, y = _data(5, S, seed=21, pad=4)
    _check(net, r, x, y, "lambdaLoss", dev, lambda_kw=kw)


def test_lambda_k0_and_empty_batch(dev):
    net = _model(dev)
    from ltr_mi355x.scorer import FusedRanker
    r = FusedRanker(net, loss="lambdaLoss", k=0)
    x, y = _data(3, 32)
    assert float(r.step(x.to(dev), y.to(dev))) == 0.0 and float(r.flat_grad.abs().max()) == 0.0
    r2 = FusedRanker(net, loss="approxNDCG")
    l = r2.step(torch.empty(0, 32, 136, device=dev), torch.empty(0, 32, device=dev))
    assert torch.isnan(l) and float(r2.flat_grad.abs().max()) == 0.0


@pytest.mark.parametrize("S", [64, 100])
def test_listnet_apply_sigmoid(dev, S):
    net = _model(dev, seed=4)
    from ltr_mi355x.scorer import FusedRanker
    r = FusedRanker(net, loss="listnet", apply_sigmoid=True)
    x, y = _data(4, S, seed=2)
    _check(net, r, x, y, "listnet", dev, apply_sigmoid=True)


@pytest.mark.parametrize("case_id", ["lambda_S32", "lambda_S100", "lambda_S128", "listnet_S32", "listnet_S100", "listnet_S128",
                                     "approx_S32", "approx_S100", "approx_S128", "lambda_F64_S100"])
def test_r6_goldens(dev, case_id):
    cases, g, gm = golden_r6()
    case = [c for c in cases if c["id"] == case_id][0]
    from architeture.multiLayer import make_model
    from ltr_mi355x.scorer import FusedRanker
    net = make_model(**copy.deepcopy(case["model"]), n_features=case["F"])
    net.load_state_dict({k: torch.from_numpy(v) for k, v in gm.weights(case).items()})
    net = net.to(dev)
    loss = {"lambdaLoss": "lambdaLoss", "listnetLoss": "listnet", "approxNDCGLoss": "approxNDCG"}[case["loss"]]
    kw = dict(weighing_scheme="ndcgLoss2PP_scheme") if loss == "lambdaLoss" else {}
    r = FusedRanker(net, loss=loss, **kw)
    x, y = (torch.from_numpy(a) for a in gm.inputs(case))
    l, got = _check(net, r, x, y, loss, dev, lambda_kw=kw or None)
    want = float(g[f"{case_id}/loss"])
    assert abs(l - want) <= 2e-5 * abs(want)
    sk = gm.sketch_vectors(case)
    top = max(float(np.abs(t).max()) for t in got)
    for k, gr in zip(case["keys"], got):
        gr = gr.astype(np.float64)
        if f"{case_id}/g/{k}" in g:
            assert np.abs(gr - g[f"{case_id}/g/{k}"]).max() <= 2e-5 * top, k
        else:
            r_in, r_out = sk[k]
            for a, b in ((gr @ r_in, g[f"{case_id}/g_in/{k}"]), (r_out @ gr, g[f"{case_id}/g_out/{k}"])):
                assert np.abs(a - b).max() <= 2e-5 * max(np.abs(b).max(), 1e-30) + 1e-6 * top, k


@pytest.mark.parametrize("S", [128, 100])
def test_deterministic(dev, S):
    net = _model(dev)
    from ltr_mi355x.scorer import FusedRanker
    r = FusedRanker(net, loss="lambdaLoss", weighing_scheme="ndcgLoss2PP_scheme")
    x, y = (t.to(dev) for t in _data(40, S, seed=1))
    r.step(x, y)
    a = r.flat.clone()
    r.step(x, y)
    assert torch.equal(a, r.flat)


def test_zero_grad_rebinding(dev):
    net = _model(dev)
    from ltr_mi355x.scorer import FusedRanker
    r = FusedRanker(net, loss="listnet")
    opt = torch.optim.SGD(net.parameters(), lr=0.1)
    x, y = (t.to(dev) for t in _data(4, 64))
    r.step(x, y)
    opt.zero_grad(set_to_none=True)
    r.step(x, y)
    assert all(p.grad is v for p, v in zip(r.params, r._grad_views))


def test_adam_training_tracks_fp64(dev):
    """20 Adam steps through FusedRanker vs the same loop on the fp64 oracle: a stale fold would drift at once."""
    net = _model(dev, seed=12)
    from ltr_mi355x.scorer import FusedRanker
    r = FusedRanker(net, loss="approxNDCG")
    ref = [p.detach().cpu().double().clone().requires_grad_(True) for p in net._ltr_params()]
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, eps=1e-6)
    opt_ref = torch.optim.Adam(ref, lr=1e-3, eps=1e-6)
    import ltr_oracle as O
    for it in range(20):
        x, y = _data(16, 128, seed=100 + it)
        l = float(r.step(x.to(dev), y.to(dev)))
        opt.step()
        opt_ref.zero_grad()
        lr_ = O.approx_ndcg(linear_forward(x, ref, SIZES, False), y.double())
        lr_.backward()
        opt_ref.step()
        assert abs(l - float(lr_.detach())) <= 1e-5 * abs(float(lr_.detach())), it
    # weight matrices (their exact gradients are not zero; the biases' are, under a shift-invariant loss, and Adam steps on noise)
    for p, q in zip(net._ltr_params(), ref):
        if p.dim() == 2:
            d = float((p.detach().cpu().double() - q.detach()).abs().max()) / float(q.detach().abs().max())
            ledger_record("Adam x20 weights / max|tensor|", d)
            assert d < 1e-5
    basis = torch.cat([torch.zeros(1, 136), torch.eye(136)]).unsqueeze(0)
    w_got = linear_forward(basis, [t.detach().cpu().double() for t in net._ltr_params()], SIZES, False)
    w_ref = linear_forward(basis, [t.detach() for t in ref], SIZES, False)
    w_got, w_ref = w_got[:, 1:] - w_got[:, :1], w_ref[:, 1:] - w_ref[:, :1]     # w_eff (the constant b_eff moves on noise)
    assert float((w_got - w_ref).abs().max()) <= 1e-5 * float(w_ref.abs().max())


def test_dropout_encoder_d_output_rules(dev):
    from ltr_mi355x import LtrDeviceError
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, seed=3, dropout=0.2)
    r = FusedRanker(net, loss="approxNDCG")
    x, y = _data(3, 64, seed=4)
    net.train()
    with pytest.raises(NotImplementedError, match="module path"):
        r.step(x.to(dev), y.to(dev))
    net.eval()
    _check(net, r, x, y, "approxNDCG", dev)
    net.train()
    _check(net, r, x, y, "approxNDCG", dev, train=False)
    with pytest.raises(NotImplementedError):
        r.step(x.to(dev), y.to(dev), keep1=torch.ones(3, 64, 128, device=dev))
    with pytest.raises(LtrDeviceError):
        r.step(x, y, train=False)
    from architeture.multiLayer import make_model
    enc = make_model(dict(sizes=[32], input_norm=False, activation=None, dropout=0.0),
                     dict(N=1, d_ff=64, h=2, dropout=0.0, positional_encoding=None), dict(d_output=1), 136).to(dev)
    with pytest.raises(NotImplementedError):
        FusedRanker(enc)
    two = make_model(dict(sizes=[32], input_norm=False, activation=None, dropout=0.0), False, dict(d_output=2), 136).to(dev)
    with pytest.raises(NotImplementedError):
        FusedRanker(two)


@pytest.mark.parametrize("S", [128, 100])
def test_precision_gain_over_module_path(dev, S):
    """The new step's gradient error against fp64 is below the module path's (bf16 GEMMs, ltr_mi355x/encoder.py)."""
    from losses.approxNDCG import approxNDCGLoss
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, seed=6)
    x, y = _data(16, S, seed=9)
    params = net._ltr_params()
    _, ref = oracle_step(params, x, y, SIZES, False, "approxNDCG")
    ref_flat = np.concatenate([g.reshape(-1) for g in ref])
    top = np.abs(ref_flat).max()
    net.zero_grad()
    approxNDCGLoss(net(x.to(dev), None, None), y.to(dev)).backward()
    mod = np.concatenate([p.grad.detach().cpu().double().numpy().reshape(-1) for p in params])
    r = FusedRanker(net, loss="approxNDCG")
    r.step(x.to(dev), y.to(dev))
    fused = r.flat_grad.detach().cpu().double().numpy()
    e_mod, e_fused = np.abs(mod - ref_flat).max() / top, np.abs(fused - ref_flat).max() / top
    print(f"[precision S={S}] gradient max|err|/max|ref|: module path {e_mod:.3e}, fused folded step {e_fused:.3e}")
    ledger_record("module path grad / max|whole gradient| (bf16)", e_mod, tol=1.0, asserted=False)
    ledger_record("fused folded grad / max|whole gradient|", e_fused)
    assert e_fused < e_mod and e_fused < 1e-5


# ------------------------------------------------------------------------------------------- every loss path in the one-launch step
def _scale_spread(net, x, sizes, input_norm, target):
    """Scale the output layer in place so that max |s_k - s_0| over the batch is `target`; returns the fp32 scores after it."""
    params = net._ltr_params()
    s = linear_forward(x, [p.detach().cpu().double() for p in params], sizes, input_norm)
    with torch.no_grad():
        params[-2].mul_(target / float((s - s[:, :1]).abs().max()))
    return linear_forward(x, [p.detach().cpu().double() for p in params], sizes, input_norm).to(torch.float32)


PATH_REGIMES = {          # regime -> (max |s_k - s_0|, paths of approx_ndcg_slate that must occur in the batch)
    "noclamp": (6.0, {"noclamp"}), "fast": (30.0, {"fast"}), "perpair": (150.0, {"perpair"}), "mixed": (150.0, {"noclamp", "fast", "perpair"}),
    "fractional": (6.0, {"fast"}), "front": (30.0, {"fast"}), "input_norm": (30.0, {"fast"}),
}


def _path_batch(regime, S):
    """(net, x, y, sizes, input_norm) of a regime: 640 documents = 5 tiles of 128, so at grid = 2 a workgroup walks 2 or 3 tiles."""
    ln = regime == "input_norm"
    F, sizes = (64, [32, 16]) if ln else (136, SIZES)
    net = _model("cpu", seed=14, F=F, sizes=sizes, input_norm=ln)
    B = 640 // S
    x, y = _data(B, S, F=F, seed=40 + S)
    g = torch.Generator().manual_seed(S)
    if ln:
        x = x * 3.0 + 1.5
    if regime == "mixed":                             # consecutive slates (and tiles) on different paths; one slate all padding
        for b in range(B):
            x[b] *= (0.02, 0.2, 1.0)[b % 3]
        y[B - 2] = -1.0
        y[1, S - 5:] = -1.0
    if regime == "fractional":
        y = y + 0.25 * torch.rand(B, S, generator=g)
        y[:, -3:] = -1.0
    if regime == "front":                             # document 0 padded: its score is the reference point of every exponential
        y[:, :3] = -1.0
        y[-1, -4:] = -1.0
    return net, x, y, sizes, ln


@pytest.mark.parametrize("S", [32, 64, 128])
@pytest.mark.parametrize("regime", list(PATH_REGIMES))
def test_approxndcg_paths_one_launch(dev, regime, S):
    """approx_ndcg_slate inside linear_fused_kernel on each of its three paths (tests/slate_loss_cases.path_of names the path of
    every slate from the fp64 scores), at the default grid and at grid = 2, where a workgroup walks several tiles of different
    paths and the label histogram has to be clean for each."""
    import slate_loss_cases as SC
    from ltr_mi355x.scorer import FusedRanker
    net, x, y, sizes, ln = _path_batch(regime, S)
    target, want = PATH_REGIMES[regime]
    s32 = _scale_spread(net, x, sizes, ln, target)
    paths = {SC.path_of(s32[b], y[b], 1.0, 1e-10, -1.0) for b in range(x.shape[0])}
    assert paths >= want and (regime in ("mixed", "perpair") or paths == want), (regime, S, paths)
    net = net.to(dev)
    for grid in (None, 2):
        r = FusedRanker(net, loss="approxNDCG", grid=grid)
        assert type(r).__name__ == "LinearFusedRanker" and (grid is None or r.grid == 2)
        _check(net, r, x, y, "approxNDCG", dev, sizes=sizes, input_norm=ln)      # the file's flat 1e-5 on loss and gradients


@pytest.mark.parametrize("S", [32, 64, 128])
@pytest.mark.parametrize("regime", ["wide", "labels30", "input_norm"])
@pytest.mark.parametrize("apply_sigmoid", [False, True])
def test_listnet_regimes_one_launch(dev, apply_sigmoid, regime, S):
    """listnet_slate inside linear_fused_kernel: score spread 60 (every q still above 1e-30), labels up to 30 (softmax(y_true)
    one-hot to fp32), an input-norm network; default grid and grid = 2."""
    from ltr_mi355x.scorer import FusedRanker
    net, x, y, sizes, ln = _path_batch("input_norm" if regime == "input_norm" else "fast", S)
    if regime == "labels30":
        y = torch.randint(0, 31, y.shape, generator=torch.Generator().manual_seed(S)).float()
    s32 = _scale_spread(net, x, sizes, ln, 30.0 if regime != "labels30" else 4.0)
    assert float(torch.softmax(s32, dim=1).min()) >= 1e-30
    net = net.to(dev)
    for grid in (None, 2):
        r = FusedRanker(net, loss="listnet", apply_sigmoid=apply_sigmoid, grid=grid)
        _check(net, r, x, y, "listnet", dev, sizes=sizes, input_norm=ln, apply_sigmoid=apply_sigmoid)


# ---------------------------------------------------------------------------------------------------------- data parallel
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, os.path.join(ROOT, "nn-with-pytorch-personalized-losses_amd"))
    dev = torch.device("cuda:0")
    net = _model(dev, seed=31)
    from ltr_mi355x.dp import QueryShardedTrainer, shard_range, sync_parameters
    from ltr_mi355x.scorer import FusedRanker
    sync_parameters(net)
    tr = QueryShardedTrainer(FusedRanker(net, loss="approxNDCG"), torch.optim.SGD(net.parameters(), lr=0.5))
    X, y = _data(11, 128, seed=77)                   # ragged shards: 6 + 5 slates
    lo, hi = shard_range(11, rank, world)
    grads = []
    for _ in range(2):
        tr.step(X[lo:hi].to(dev), y[lo:hi].to(dev))
        grads.append(tr.local.flat_grad.detach().cpu().clone())
    torch.save({"grads": grads, "params": [p.detach().cpu() for p in net._ltr_params()]}, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_equal_single_rank(dev):
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_dp_worker, args=(2, _free_port(), d), nprocs=2, join=True)
        r0 = torch.load(os.path.join(d, "rank0.pt"), weights_only=True)
        r1 = torch.load(os.path.join(d, "rank1.pt"), weights_only=True)
    from ltr_mi355x.scorer import FusedRanker
    net = _model(dev, seed=31)
    r = FusedRanker(net, loss="approxNDCG")
    opt = torch.optim.SGD(net.parameters(), lr=0.5)
    X, y = _data(11, 128, seed=77)
    for it in range(2):
        r.step(X.to(dev), y.to(dev))
        ref = r.flat_grad.detach().cpu().clone()
        opt.step()
        for got in (r0["grads"][it], r1["grads"][it]):
            assert float((got - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    for a, b in zip(r0["params"], [p.detach().cpu() for p in net._ltr_params()]):
        assert float((a - b).abs().max()) <= 1e-5 * max(float(b.abs().max()), 1e-6)
