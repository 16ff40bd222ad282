"""GPU: the persistent kernels' multi-tile loops against the fp64 oracle.

Every FC training kernel walks 128-document super-tiles, `st = blockIdx.x; st += gridDim.x`, and carries state from one tile to
the next: the dW accumulators, the next tile's X (issued under dW2 by the 136-wide backward / fused kernels), the f16 x 2 variant's
running-maximum exponents, and LDS contracts such as approx_ndcg_slate's zeroed label bins.  At the production grid (one or two
workgroups per CU) a test needs 32 768+ documents before any workgroup runs a second tile, so the cases here force the grid instead
(FusedRanker(grid=...), LinearFusedRanker(grid=...), scorer.cu_count patched for the module path): a few dozen slates then give
every workgroup up to 10 tiles, ordered so that one workgroup meets mixed loss regimes, padding, fractional labels and X scales
that rise and fall from tile to tile.  Bars are the suite's: 1e-5 on the loss, assert_grads (max(1e-5, 4 x the fp32 oracle's own
noise) per tensor) on every gradient, the risk file's floors for the risk step.  The launchers are wrapped to record the grid each
launch received, so every case also proves how many tiles per workgroup it ran."""
import math

import numpy as np
import pytest
import torch

import ltr_oracle as O
from conftest import ledger_record
from conftest import relerr as _relerr
from test_fused_gaps_gpu import _exported_masks
from test_linear_fused_cpu import oracle_step as linear_oracle_step
from test_linear_fused_gpu import SIZES as LINEAR_SIZES
from test_linear_fused_gpu import _model as linear_model
from test_risk_fused_gpu import _assert_grads as risk_assert_grads
from test_risk_fused_gpu import _assert_loss as risk_assert_loss
from test_risk_fused_gpu import _data as risk_data
from test_risk_fused_gpu import _net as risk_net
from test_risk_fused_gpu import _oracle as risk_oracle
from test_scorer_gpu import LAMBDA_KW, _grads, assert_grads

pytestmark = pytest.mark.gpu
TOL = 1e-5
TILE = 128
LOSSES = ["approxNDCG", "listnet", "lambdaLoss"]
# X scale 2^e of super-tile t (t mod 10).  Grid 1 runs them in order; grid 3 gives workgroup 0 the tiles 0, 3, 6, 9 (2^0, 2^6,
# 2^-5, 2^2), workgroup 1 the tiles 1, 4, 7 (2^-6, 2^4, 2^-2), workgroup 2 the tiles 2, 5, 8 (2^5, 2^-3, 2^6): every workgroup sees
# the scale rise and fall, and a later tile larger than any before it (the f16 x 2 accumulator rescale, with accumulators held).
TILE_EXP = [0, -6, 5, 6, 4, -3, -5, -2, 6, 2]
# slates per case: 10 super-tiles at every slate length (4 / 3 / 3 tiles per workgroup at grid 3), the last one partial for S < 128
B_OF_S = {32: 37, 64: 19, 128: 10}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    return torch.device("cuda:0")


def _f16x2():
    import ltr_mi355x
    return ltr_mi355x.library_path().endswith("_f16x2.so")


def _tiles(n_docs):
    return (n_docs + TILE - 1) // TILE


# ------------------------------------------------------------------------------------------------------ launch records
class Launches:
    """Wraps the persistent launchers of lib() and records (entry, documents, grid) of every launch."""
    ENTRIES = {
        "ltr_fused_step": lambda a: (a[4] * a[5], a[-2]),
        "ltr_fused_step_lambda": lambda a: (a[3] * a[4], a[-2]),
        "ltr_mlp_forward": lambda a: (a[2], a[-2]),
        "ltr_mlp_backward": lambda a: (a[2], a[-2]),
        "ltr_mlp_forward_save": lambda a: (a[2], a[-2]),
        "ltr_mlp_backward_saved": lambda a: (a[2], a[-2]),
        "ltr_linear_fused_step": lambda a: (a[3] * a[4], a[-2]),
    }

    def __init__(self, monkeypatch):
        from ltr_mi355x import lib
        h = lib()
        self.calls = []
        for name, decode in self.ENTRIES.items():
            fn = getattr(h, name)

            def wrapped(*args, _fn=fn, _name=name, _decode=decode):
                n, grid = _decode(args)
                self.calls.append((_name, int(n), int(grid)))
                return _fn(*args)
            monkeypatch.setattr(h, name, wrapped)

    def reset(self):
        self.calls = []

    def assert_tiles(self, entries, per_wg, grid=None):
        """Every launch of `entries` ran at least `per_wg` super-tiles on some workgroup (ceil(n_super / grid)), at `grid` if given."""
        seen = [c for c in self.calls if c[0] in entries]
        assert seen, (entries, self.calls)
        for name, n, g in seen:
            if grid is not None:
                assert g == grid, (name, g, grid)
            assert math.ceil(_tiles(n) / min(g, _tiles(n))) >= per_wg, (name, n, g, per_wg)
        return seen


# ------------------------------------------------------------------------------------------------------ networks / oracle
KINDS = ["double136_eval", "double136_train", "triple136_fold", "triple136_layers", "two64", "double64", "triple64_fold"]
KIND_NET = {"double136_eval": ("double", 136), "double136_train": ("double", 136), "triple136_fold": ("triple", 136),
            "triple136_layers": ("triple", 136), "two64": ("two", 136), "double64": ("double", 64), "triple64_fold": ("triple", 64)}
# which persistent kernel runs the one-launch step: the generic slate pipeline (ltr_scorer.hip) or the document-split fcw kernel
KIND_FAMILY = {"double136_eval": "pipeline", "double136_train": "pipeline", "triple136_fold": "fcw", "triple136_layers": "pipeline",
               "two64": "fcw", "double64": "pipeline", "triple64_fold": "pipeline"}
LAST = {"double": "fc3.weight", "triple": "l3.weight", "two": "fc4.weight"}


def _net(kind, monkeypatch, seed=7):
    from architeture.doubleLayer import DoubleLayerNet
    from architeture.tripleLayer import TripleLayerNet
    from ltr_mi355x.extra_nets import TwoLayerNet
    monkeypatch.setenv("LTR_TRIPLE_FOLD", "0" if kind == "triple136_layers" else "1")
    arch, F = KIND_NET[kind]
    torch.manual_seed(seed)
    net = {"double": DoubleLayerNet, "triple": TripleLayerNet, "two": TwoLayerNet}[arch](F)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    return net, sd, arch, F


def _scores(arch, x, p, k1=None, k2=None):
    if arch == "triple":
        return O.triple_layer_forward(x, p).squeeze(-1)
    if arch == "two":
        return O.two_layer_forward(x, p).squeeze(-1)
    return O.double_layer_forward(x, p, k1, k2).squeeze(-1)


def _oracle(arch, sd, x, y, loss, keep=(None, None), dtype=torch.float64):
    p = {k: v.to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    k1, k2 = (None if k is None else k.to(dtype) for k in keep)
    s = _scores(arch, x.to(dtype), p, k1, k2)
    yd = y.to(dtype)
    if loss == "approxNDCG":
        l = O.approx_ndcg(s, yd)
    elif loss == "listnet":
        l = O.listnet(yd, s)
    else:
        l = O.lambda_loss(s, yd, **LAMBDA_KW)
    l.backward()
    return float(l.detach()), {k: v.grad.numpy() for k, v in p.items()}, s.detach()


def _ranker(net, loss, grid):
    from ltr_mi355x.scorer import FusedRanker
    kw = dict(weighing_scheme="ndcgLoss2PP_scheme") if loss == "lambdaLoss" else {}
    return FusedRanker(net, loss=loss, grid=grid, **kw)


def _spread(s, y):
    """Per slate: max over real documents of |s_k - s_0| -- what approx_ndcg_fused decides its path on (<= 8 with integer labels:
    no-clamp; <= 69: fast; beyond: per-pair exponentials)."""
    real = y >= 0
    d = (s - s[:, :1]).abs()
    return torch.where(real, d, torch.zeros_like(d)).amax(dim=1)


def _regimes(s, y):
    sp = _spread(s, y)
    integer = ((y.clamp(min=0) == y.clamp(min=0).floor()) | (y < 0)).all(dim=1)
    real = (y >= 0).any(dim=1)
    out = []
    for b in range(y.shape[0]):
        if not real[b]:
            out.append("empty")
        elif sp[b] < 7.0 and integer[b]:
            out.append("noclamp")
        elif sp[b] < 60.0 and (sp[b] > 10.0 or not integer[b]):
            out.append("fast")
        elif sp[b] > 80.0:
            out.append("perpair")
        else:
            out.append("border")
    return out


def _tie_gap(s64, s32, y):
    """Per slate, the smallest gap between two real documents' fp64 scores over the fp32 restatement's largest score error in that
    slate; the minimum over slates.  lambdaLoss weighs pairs by predicted RANKS, and a pair closer than fp32 resolves ranks either
    way in any fp32 implementation."""
    worst = float("inf")
    for b in range(y.shape[0]):
        real = y[b] >= 0
        v = s64[b][real].sort().values
        if v.numel() > 1:
            err = float((s32[b][real].double() - s64[b][real]).abs().max())
            worst = min(worst, float((v[1:] - v[:-1]).min()) / max(err, 1e-30))
    return worst


def _mixed(B, S, F, seed, cap=6):
    """Slates whose 128-document tiles carry X scales 2^TILE_EXP[t] (clipped to 2^+-cap), with padded tails, an all-padding slate and
    one slate of fractional labels."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, S, F, generator=gen)
    y = torch.randint(0, 5, (B, S), generator=gen).float()
    tile = (torch.arange(B) * S) // TILE
    x *= torch.tensor([2.0 ** max(-cap, min(cap, TILE_EXP[int(t) % len(TILE_EXP)])) for t in tile]).view(B, 1, 1)
    y[1, S - S // 4:] = -1.0                        # padded tails
    y[B // 2, S - 5:] = -1.0
    y[B - 1, S // 2:] = -1.0
    y[2] = -1.0                                     # a slate of padding only
    y[B - 3] += 0.25 * torch.rand(S, generator=gen)  # fractional labels
    return x, y


def _case_data(kind, loss, B, S, sd, arch, F, keep_fn=None):
    """Mixed-order data; approxNDCG: the last layer scaled so that the 2^6 tiles take the per-pair path (the smaller ones the fast
    and no-clamp paths, the recipe of test_fused_approxndcg_every_path's mixed_slates); lambdaLoss: the first tie-free seed -- with X
    scales up to 2^6 where one exists, else up to 2^3 (TripleLayerNet's sigmoids saturate at 2^6: whole slates of documents then share
    hidden patterns and tie in score)."""
    for i in range(128):
        seed, cap = 1000 * S + B + i % 64, (6 if i < 64 else 3)
        x, y = _mixed(B, S, F, seed, cap)
        keep = keep_fn(B, S) if keep_fn else (None, None)
        sd_case = dict(sd)
        if loss == "approxNDCG":
            s = _scores(arch, x.double(), {k: v.double() for k, v in sd.items()}, *[None if k is None else k.double() for k in keep])
            sd_case[LAST[arch]] = sd[LAST[arch]] * (150.0 / float(_spread(s, y).max()))
            return x, y, sd_case, keep
        if loss != "lambdaLoss":
            return x, y, sd_case, keep
        p64 = {k: v.double() for k, v in sd.items()}
        s64 = _scores(arch, x.double(), p64, *[None if k is None else k.double() for k in keep])
        s32 = _scores(arch, x, sd, *keep)
        if _tie_gap(s64, s32, y) > 8.0:
            return x, y, sd_case, keep
    raise AssertionError("no tie-free seed")


def _record_family(family, grid, got, rg, rg32=None):
    """Ledger: the largest per-tensor gradient error of this case under one name per kernel family and grid."""
    top = max(float(np.abs(v).max()) for v in rg.values())
    worst, noise = 0.0, 0.0
    for k, v in got.items():
        r = np.asarray(rg[k], dtype=np.float64)
        rmax = float(np.abs(r).max())
        if rmax < 1e-3 * top:
            continue
        worst = max(worst, float(np.abs(np.asarray(v, dtype=np.float64) - r).max()) / rmax)
        if rg32 is not None:
            noise = max(noise, float(np.abs(np.asarray(rg32[k], dtype=np.float64) - r).max()) / rmax)
    ledger_record(f"persistent tiles {family} grid={grid}: grad / max|tensor|", worst, noise if rg32 is not None else None, TOL)


def _loss_ok(out, rl, what):
    e = _relerr(np.asarray(float(out)), np.asarray(rl))
    ledger_record(f"persistent tiles {what}: loss", e)
    assert e < TOL, (float(out), rl, e)


def _same_loss(a, b, what, scorer_kernel=True):
    """Per-slate scores and losses do not depend on which workgroup ran a tile -- except in the f16 x 2 variant, whose X images are
    scaled by the workgroup's RUNNING maximum exponent (ltr_scorer.hip convert_x / ltr_fcw.h): a tile's hi / lo split, and so its
    scores, depend on the tiles that workgroup ran before.  There the two grids agree at the parity bar instead."""
    a, b = float(a), float(b)
    if scorer_kernel and _f16x2():
        e = abs(a - b) / max(abs(b), 1e-30)
        ledger_record(f"persistent tiles {what}: loss forced grid vs default grid (f16 x 2)", e)
        assert e < TOL, (a, b)
    else:
        assert a == b or (math.isnan(a) and math.isnan(b)), (what, a, b)


# ------------------------------------------------------------------------------------------------------ 1. one-launch step
CASES = [(k, S) for k in KINDS for S in (32, 128)] + [("double136_eval", 64)]


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("kind,S", CASES)
def test_fused_step_forced_grid(kind, S, loss, grid, dev, monkeypatch):
    net, sd, arch, F = _net(kind, monkeypatch)
    B = B_OF_S[S]
    seed = 0x5EED0000 + 17 * S + B if kind == "double136_train" else None
    keep_fn = (lambda B_, S_: _exported_masks(seed, B_ * S_, dev, B_, S_)) if seed is not None else None
    x, y, sd, keep = _case_data(kind, loss, B, S, sd, arch, F, keep_fn)
    if loss == "approxNDCG":
        s = _scores(arch, x.double(), {k: v.double() for k, v in sd.items()}, *[None if k is None else k.double() for k in keep])
        seen = set(_regimes(s, y))
        assert {"noclamp", "fast", "perpair", "empty"} <= seen, seen
    net.load_state_dict(sd)
    net = net.to(dev)
    net.train() if seed is not None else net.eval()
    rec = Launches(monkeypatch)
    r = _ranker(net, loss, grid)
    out = r.step(x.to(dev), y.to(dev), seed=seed).clone()
    got = {k: v.copy() for k, v in _grads(net).items()}
    n_super = _tiles(B * S)
    assert n_super == 10 and (S == 128 or B * S % TILE)           # ragged 4 / 3 / 3 at grid 3; a partial last tile for S < 128
    rec.assert_tiles(("ltr_fused_step", "ltr_fused_step_lambda"), math.ceil(n_super / grid), grid)
    rl, rg, _ = _oracle(arch, sd, x, y, loss, keep)
    _, rg32, _ = _oracle(arch, sd, x, y, loss, keep, dtype=torch.float32)
    family = KIND_FAMILY[kind]
    _loss_ok(out, rl, f"{family} grid={grid}")
    _record_family(family, grid, got, rg, rg32)
    assert_grads(got, rg, ref32=rg32)
    out0 = _ranker(net, loss, None).step(x.to(dev), y.to(dev), seed=seed)
    _same_loss(out, out0, f"{family} {kind} S={S} {loss}")


# ------------------------------------------------------------------------------------------------------ 2. three-launch and module paths
@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("loss", ["approxNDCG", "lambdaLoss"])
@pytest.mark.parametrize("kind,S", [("double136_eval", 100), ("double136_eval", 512), ("triple136_fold", 100), ("triple136_fold", 512)])
def test_three_launch_path_forced_grid(kind, S, loss, grid, dev, monkeypatch):
    """Slates of 100 / 512 documents cross the 128-document tiles: forward (activations saved) and backward launches at a forced
    grid, 11 / 12 tiles."""
    net, sd, arch, F = _net(kind, monkeypatch, seed=23)
    B = {100: 13, 512: 3}[S]
    x, y, sd, _ = _case_data(kind, loss, B, S, sd, arch, F)
    net.load_state_dict(sd)
    net = net.to(dev).eval()
    rec = Launches(monkeypatch)
    out = _ranker(net, loss, grid).step(x.to(dev), y.to(dev)).clone()
    got = {k: v.copy() for k, v in _grads(net).items()}
    n_super = _tiles(B * S)
    assert n_super >= 11
    rec.assert_tiles(("ltr_mlp_forward_save", "ltr_mlp_backward_saved"), math.ceil(n_super / grid), grid)
    rl, rg, _ = _oracle(arch, sd, x, y, loss)
    _, rg32, _ = _oracle(arch, sd, x, y, loss, dtype=torch.float32)
    _loss_ok(out, rl, f"three-launch grid={grid}")
    _record_family("three-launch", grid, got, rg, rg32)
    assert_grads(got, rg, ref32=rg32)
    out0 = _ranker(net, loss, None).step(x.to(dev), y.to(dev))
    assert float(out) == float(out0), (float(out), float(out0))     # the forward launch computes each document's score on its own


@pytest.mark.parametrize("kind,saved", [("double", False), ("triple", False), ("double", True)])
def test_module_path_two_workgroups(kind, saved, dev, monkeypatch):
    """net(x) + loss + backward() with scorer.cu_count patched to 2: default_grid gives the forward and backward launches two
    workgroups for 17 tiles (9 / 8 each).  saved=True: DoubleLayerNet with dropout p = 0.3 in training mode, whose forward keeps
    the hidden activations for the backward launch (ltr_mlp_forward_save / ltr_mlp_backward_saved), against the exported masks."""
    from losses.approxNDCG import approxNDCGLoss
    from ltr_mi355x import scorer
    monkeypatch.setenv("LTR_TRIPLE_FOLD", "1")
    monkeypatch.setattr(scorer, "cu_count", lambda device: 2)
    net, sd, arch, F = _net(kind + "136_eval" if kind == "double" else "triple136_fold", monkeypatch, seed=29)
    B, S = 21, 100
    x, y = _mixed(B, S, F, 4242)
    net = net.to(dev)
    rec = Launches(monkeypatch)
    keep = (None, None)
    if saved:
        p, seed = 0.3, 0x0DDBA11C0FFEE123
        net.train()
        scores = scorer.mlp_scores(net._ltr_net, net._ltr_params(), x.to(dev), dropout=scorer.drop_code(True, p), seed=seed)
        keep = tuple(scorer.dropout_keep_mask(seed, i, B * S, F, dev, p=p).cpu().float().view(B, S, F) for i in (0, 1))
        entries = ("ltr_mlp_forward_save", "ltr_mlp_backward_saved")
    else:
        p = 0.5
        net.eval()
        scores = net(x.to(dev), None, None)
        entries = ("ltr_mlp_forward", "ltr_mlp_backward")
    loss = approxNDCGLoss(scores.squeeze(-1), y.to(dev))
    loss.backward()
    seen = rec.assert_tiles(entries, 9, 2)
    assert {c[0] for c in seen} == set(entries), seen
    pd = {k: v.double().clone().requires_grad_(True) for k, v in sd.items()}
    p32 = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    refs = []
    for pp, dt in ((pd, torch.float64), (p32, torch.float32)):
        k1, k2 = (None if k is None else k.to(dt) for k in keep)
        s = (O.triple_layer_forward(x.to(dt), pp) if arch == "triple" else O.double_layer_forward(x.to(dt), pp, k1, k2, p)).squeeze(-1)
        l = O.approx_ndcg(s, y.to(dt))
        l.backward()
        refs.append((float(l.detach()), s.detach(), {k: v.grad.numpy() for k, v in pp.items()}))
    (rl, rs, rg), (_, _, rg32) = refs
    e = _relerr(scores.detach().squeeze(-1).cpu().numpy(), rs.numpy())
    ledger_record(f"persistent tiles module path grid=2 ({'saved' if saved else 'recomputing'} backward): scores", e)
    assert e < TOL
    _loss_ok(loss.detach(), rl, "module path grid=2")
    got = _grads(net)
    _record_family("module path", 2, got, rg, rg32)
    assert_grads(got, rg, ref32=rg32)


# ------------------------------------------------------------------------------------------------------ 3. linear FusedRanker
def _linear_check(net, ranker, x, y, loss, dev, what):
    kw = dict(weighing_scheme="ndcgLoss2PP_scheme") if loss == "lambdaLoss" else None
    out = ranker.step(x.to(dev), y.to(dev)).clone()
    params = net._ltr_params()
    got = {str(i): p.grad.detach().cpu().numpy().copy() for i, p in enumerate(params)}
    rl, rg = linear_oracle_step(params, x, y, LINEAR_SIZES, False, loss, lambda_kw=kw)
    _, rg32 = linear_oracle_step(params, x, y, LINEAR_SIZES, False, loss, dtype=torch.float32, lambda_kw=kw)
    rg, rg32 = ({str(i): g for i, g in enumerate(gs)} for gs in (rg, rg32))
    _loss_ok(out, rl, what)
    _record_family(what, ranker.grid, got, rg, rg32)
    assert_grads(got, rg, ref32=rg32)
    return out


def _linear_spread(net, x, y, target):
    """Scale the config network's output layer so that the largest slate score spread is `target` (the folded network is affine: the
    spread follows the X scale exactly)."""
    import test_linear_fused_cpu as C
    s = C.linear_forward(x, [p.detach().cpu().double() for p in net._ltr_params()], LINEAR_SIZES, False)
    with torch.no_grad():
        net.output_layer.w_1.weight.mul_(target / float(_spread(s, y).max()))
    return C.linear_forward(x, [p.detach().cpu().double() for p in net._ltr_params()], LINEAR_SIZES, False)


def _linear_case(dev, loss, B, S, seed):
    """The config network with the mixed tile order.  approxNDCG: spread 150, so that the 2^6 tiles take the per-pair path.  The
    others: spread 40 -- unscaled, this network's 2^6 tiles spread their scores by more than 100, where the softmax of ListNet (whose
    log is taken literally, listnet.py:16) underflows to 0 in fp32 and the loss is +inf in the reference's own arithmetic."""
    net = linear_model(dev, seed=5)
    x, y = _mixed(B, S, 136, seed)
    s = _linear_spread(net, x, y, 150.0 if loss == "approxNDCG" else 40.0)
    if loss == "approxNDCG":
        assert {"noclamp", "fast", "perpair", "empty"} <= set(_regimes(s, y))
    return net, x, y


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("S", [32, 64, 128])
def test_linear_fused_step_forced_grid(S, loss, grid, dev, monkeypatch):
    """ltr_linear_fused_step (csrc/ltr_linear.hip) over 10 tiles per workgroup (grid 1) or 4 / 3 / 3 (grid 3): the dot-product
    accumulators, and the approxNDCG label-histogram bins that the kernel zeroes ONCE before its tile loop and every slate must
    leave zeroed (ltr_slate_losses.h approx_ndcg_slate)."""
    B = B_OF_S[S]
    net, x, y = _linear_case(dev, loss, B, S, 77 + S)
    rec = Launches(monkeypatch)
    r = _ranker(net, loss, grid)
    assert type(r).__name__ == "LinearFusedRanker"
    out = _linear_check(net, r, x, y, loss, dev, "linear")
    rec.assert_tiles(("ltr_linear_fused_step",), math.ceil(10 / grid), grid)
    _same_loss(out, _ranker(net, loss, None).step(x.to(dev), y.to(dev)), f"linear S={S} {loss}", scorer_kernel=False)


@pytest.mark.parametrize("grid", [1, 3])
@pytest.mark.parametrize("loss", LOSSES)
def test_linear_any_slate_forced_grid(loss, grid, dev):
    """S = 300: scores + loss kernel + ltr_linear_grad_partials, whose `grid` workgroups take contiguous document ranges."""
    net, x, y = _linear_case(dev, loss, 5, 300, 300)
    r = _ranker(net, loss, grid)
    out = _linear_check(net, r, x, y, loss, dev, "linear any-slate")
    assert float(out) == float(_ranker(net, loss, None).step(x.to(dev), y.to(dev)))


# ------------------------------------------------------------------------------------------------------ 4. risk step
@pytest.mark.parametrize("S", [100, 128])
@pytest.mark.parametrize("geom", ["double136", "triple136"])
@pytest.mark.parametrize("name", ["geoRiskLambdaLoss", "tRiskListnetLoss"])
def test_risk_step_forced_grid(name, geom, S, dev, monkeypatch):
    """The risk step's scorer launches (forward with saved activations, backward) at grid 2 over 17 / 14 tiles, against the fp64
    risk oracle at test_risk_fused_gpu's floors."""
    from ltr_mi355x.scorer import FusedRanker
    monkeypatch.setenv("LTR_TRIPLE_FOLD", "1")
    net, sd, F = risk_net(geom, dev)
    B = 17
    x, y, yb = risk_data(name, B, S, F, seed=31 * S)
    rec = Launches(monkeypatch)
    r = FusedRanker(net, loss=name, risk_args={}, grid=2)
    out = float(r.step(x.to(dev), y.to(dev), y_base=yb.to(dev)))
    n_super = _tiles(B * S)
    rec.assert_tiles(("ltr_mlp_forward_save", "ltr_mlp_backward_saved"), math.ceil(n_super / 2), 2)
    args = dict(r.risk.args)
    rl, rg = risk_oracle(name, geom, sd, x, y, yb, args)
    rl32, rg32 = risk_oracle(name, geom, sd, x, y, yb, args, dtype=torch.float32)
    risk_assert_loss(name, out, rl, rl32)
    got = {k: p.grad.detach().cpu().numpy().copy() for k, p in net.named_parameters()}
    _record_family("risk", 2, got, rg, rg32)
    risk_assert_grads(name, got, rg, rg32)
    out0 = float(FusedRanker(net, loss=name, risk_args={}).step(x.to(dev), y.to(dev), y_base=yb.to(dev)))
    assert out == out0, (out, out0)


# ------------------------------------------------------------------------------------------------------ 5. stale workspace, idle workgroups
def _family_net(family, dev, monkeypatch):
    if family == "linear":
        return linear_model(dev, seed=5), 136
    net, _, _, F = _net({"pipeline": "double136_eval", "fcw": "triple136_fold"}[family], monkeypatch, seed=41)
    return net.to(dev).eval(), F


@pytest.mark.parametrize("S", [32, 128])
@pytest.mark.parametrize("loss", ["approxNDCG", "lambdaLoss"])
@pytest.mark.parametrize("family", ["pipeline", "fcw", "linear"])
def test_idle_workgroups_leave_no_stale_partials(family, loss, S, dev, monkeypatch):
    """A large step first (every one of the 6 workgroups writes non-zero partials), then a 3-tile step at the same grid: the 3 idle
    workgroups must overwrite their stale partials with zeros.  Bit-identical to a fresh ranker's step."""
    net, F = _family_net(family, dev, monkeypatch)
    G = 6
    big_x, big_y = _mixed(4 * G * TILE // S, S, F, 5)
    x, y = _mixed(3 * TILE // S, S, F, 6)
    stale = _ranker(net, loss, G)
    stale.step(big_x.to(dev), big_y.to(dev))
    parts = stale.fold_partials[:G * stale.fold.partial_floats] if family == "fcw" else stale.partials
    assert float(parts.abs().view(G, -1).amax(dim=1).min()) > 0        # every workgroup left non-zero partials
    stale.step(x.to(dev), y.to(dev))
    a = stale.flat.clone()
    fresh = _ranker(net, loss, G)
    fresh.step(x.to(dev), y.to(dev))
    assert torch.equal(a, fresh.flat)
    assert bool(torch.isfinite(a).all()) and float(a[:-1].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------ 6. bounds
@pytest.mark.parametrize("S", [32, 100])
@pytest.mark.parametrize("loss", ["approxNDCG", "listnet", "lambdaLoss"])
@pytest.mark.parametrize("family", ["pipeline", "fcw", "linear"])
def test_nan_tail_past_the_batch_is_never_read(family, loss, S, dev, monkeypatch):
    """X and y are prefix views of buffers whose next 2.5 tiles are NaN (B * S not a multiple of 128): no launch may read past the
    batch, so the step is finite and bit-identical to the step on clean copies."""
    from ltr_mi355x.scorer import _docs
    net, F = _family_net(family, dev, monkeypatch)
    B = {32: 37, 100: 13}[S]
    n = B * S
    assert n % TILE
    x, y = _mixed(B, S, F, 9)
    if family == "linear":
        _linear_spread(net, x, y, 40.0)
    tail = 2 * TILE + TILE // 2
    xbuf = torch.full(((n + tail) * F,), float("nan"), device=dev)
    ybuf = torch.full((n + tail,), float("nan"), device=dev)
    xbuf[:n * F] = x.reshape(-1).to(dev)
    ybuf[:n] = y.reshape(-1).to(dev)
    xv, yv = xbuf[:n * F].view(B, S, F), ybuf[:n].view(B, S)
    r = _ranker(net, loss, 3)
    if family != "linear":
        assert _docs(xv, r.info).data_ptr() == xbuf.data_ptr()   # the kernels see this buffer, NaN tail included
    r.step(xv, yv)
    got = r.flat.clone()
    r.step(x.to(dev).clone(), y.to(dev).clone())
    assert bool(torch.isfinite(got).all()), got
    assert torch.equal(got, r.flat)


# ------------------------------------------------------------------------------------------------------ 7. production grid
@pytest.mark.parametrize("loss", ["listnet", "lambdaLoss"])
def test_default_grid_production_regime(loss, dev, monkeypatch):
    """DoubleLayerNet (eval) at B = ceil(3.5 x CUs) slates of 128 with the real grid: 3 and 4 tiles per workgroup."""
    from ltr_mi355x import scorer
    net, sd, arch, F = _net("double136_eval", monkeypatch, seed=3)
    net = net.to(dev).eval()
    cus = scorer.cu_count(dev)
    B, S = math.ceil(3.5 * cus), 128
    gen = torch.Generator().manual_seed(B)
    x = torch.randn(B, S, F, generator=gen)
    y = torch.multinomial(torch.tensor([0.52, 0.32, 0.13, 0.02, 0.01]), B * S, replacement=True, generator=gen).view(B, S).float()
    y[B // 3, S - 9:] = -1.0
    rec = Launches(monkeypatch)
    r = _ranker(net, loss, None)
    out = r.step(x.to(dev), y.to(dev)).clone()
    got = {k: v.copy() for k, v in _grads(net).items()}
    rec.assert_tiles(("ltr_fused_step", "ltr_fused_step_lambda"), 4, cus)
    rl, rg, _ = _oracle(arch, sd, x, y, loss)
    _, rg32, _ = _oracle(arch, sd, x, y, loss, dtype=torch.float32)
    _loss_ok(out, rl, "pipeline default grid")
    _record_family("pipeline", "default", got, rg, rg32)
    assert_grads(got, rg, ref32=rg32)
