"""GPU: the key-tiled attention kernels that carry the set-transformer scorer past 512 documents per slate (513 <= S <= 2048;
csrc/ltr_attention_tiled.h, include/ltr_encoder.h).

  * kernel parity against fp64 references built on the device (ctx at the 1e-2 bar of test_attention_fwd_bwd, dq / dk / dv at
    1.5e-2, lse2 against log2-sum-exp of the reference scores), dropout checked under the masks ltr_enc_attn_dropout_mask exports;
  * the tiled pair against the whole-row kernels where both apply (S <= 512, through the explicit _tiled entries);
  * bit-reproducibility, p_attn, the whole network (train mode under exported masks; eval mode against a reference golden at
    S = 1000), the standalone blocks, a graphed training step, and the limits.
The whole-row path (S <= 512) keeps its own tests in tests/test_encoder_gpu.py."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from conftest import ledger_record, relerr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def enc():
    from ltr_mi355x import encoder
    return encoder


def bits(t):
    return t.to(torch.bfloat16).view(torch.int16)


def unbits(t):
    return t.view(torch.bfloat16).double()


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(torch.bfloat16).double()


def err(a, b, floor=1e-30):
    a, b = a.double(), b.double()
    return float((a - b).abs().max()) / max(float(b.abs().max()), floor)


def _L():
    from ltr_mi355x._lib import lib
    from ltr_mi355x.functional import _ptr, _stream
    return lib(), _ptr, _stream


def _fwd(entry, qkv16, mask, B, S, h, dk, p, seed, sid, lse=True):
    lib, _ptr, _stream = _L()
    d = h * dk
    ctx = torch.empty(B * S, d, dtype=torch.int16, device=DEV)
    lse_t = torch.full((B * h, S), float("nan"), device=DEV) if lse else None
    args = [_ptr(qkv16), _ptr(mask), B, S, h, dk, float(p), seed, sid, _ptr(ctx)]
    if entry != "ltr_enc_attention_fwd":
        args.append(_ptr(lse_t))
    rc = getattr(lib, entry)(*args, _stream())
    assert rc == 0, (entry, rc)
    return ctx, lse_t


def _bwd(entry, qkv16, ctx, dctx16, lse, mask, B, S, h, dk, p, seed, sid):
    lib, _ptr, _stream = _L()
    dqkv = torch.empty(B * S, 3 * h * dk, dtype=torch.int16, device=DEV)
    rc = getattr(lib, entry)(_ptr(qkv16), _ptr(ctx), _ptr(dctx16), _ptr(lse), _ptr(mask), B, S, h, dk, float(p), seed, sid, _ptr(dqkv),
                             _stream())
    assert rc == 0, (entry, rc)
    return dqkv


def _reference(qkv16, mask, B, S, h, dk, p, keep, dctx16):
    """fp64 attention (transformer.py:145-164) on the bf16 operands: ctx, dqkv (autograd) and log2-sum-exp of the scores, for
    the slates that have an unmasked document (the reference yields NaN for the others; the kernels zeros)."""
    d = h * dk
    okb = [b for b in range(B) if mask is None or not bool((mask[b] == 1).all())]
    rows = torch.cat([torch.arange(b * S, (b + 1) * S, device=DEV) for b in okb])
    qr = unbits(qkv16)[rows].clone().requires_grad_(True)
    nb = len(okb)
    q, k, v = (qr[:, j * d:(j + 1) * d].view(nb, S, h, dk).transpose(1, 2) for j in range(3))
    pad = torch.zeros(nb, 1, 1, S, dtype=torch.bool, device=DEV) if mask is None else (mask[okb] == 1).view(nb, 1, 1, S)
    sc = (q @ k.transpose(-2, -1) / math.sqrt(dk)).masked_fill(pad, float("-inf"))
    lse2 = (torch.logsumexp(sc, -1) / math.log(2.0)).detach()
    pa = torch.softmax(sc, dim=-1)
    if keep is not None:
        pa = pa * keep[okb] / (1 - p)
    want = (pa @ v).transpose(1, 2).reshape(nb * S, d)
    want.backward(unbits(dctx16)[rows])
    return okb, rows, want.detach(), qr.grad, lse2


def _check_against_reference(enc, qkv16, mask, B, S, h, dk, p, seed, sid, ctx, lse, dqkv, dctx16):
    keep = enc.attn_dropout_mask(seed, sid, B, S, h, p, DEV).double() if p else None
    okb, rows, want, want_g, want_lse = _reference(qkv16, mask, B, S, h, dk, p, keep, dctx16)
    d = h * dk
    e_ctx = err(unbits(ctx)[rows], want)
    assert e_ctx < 1e-2, ("ctx", e_ctx)
    got_lse = lse.view(B, h, S)[okb].double()
    live = torch.isfinite(want_lse)
    assert torch.all(torch.isinf(got_lse[~live]) & (got_lse[~live] > 0))
    e_lse = float((got_lse[live] - want_lse[live]).abs().max()) / max(1.0, float(want_lse[live].abs().max()))
    assert e_lse < 2e-5, ("lse2", e_lse)
    got = unbits(dqkv)
    e_g = {}
    for j, name in enumerate("qkv"):
        e_g[name] = err(got[rows, j * d:(j + 1) * d], want_g[:, j * d:(j + 1) * d])
        assert e_g[name] < 1.5e-2, (f"d{name}", e_g[name])
    for b in range(B):
        if b not in okb:
            assert float(unbits(ctx)[b * S:(b + 1) * S].abs().max()) == 0.0
            assert float(got[b * S:(b + 1) * S].abs().max()) == 0.0
            assert torch.all(torch.isinf(lse.view(B, h, S)[b]))
    return e_ctx, max(e_g.values())


_HEADS = {8: 1, 16: 1, 17: 8, 24: 1, 32: 1}      # h * dk % 8 == 0 with the fewest heads (dk 17: 34-byte head slices)


# ------------------------------------------------------------------------------------------------- 1. parity vs fp64
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dk", [8, 16, 17, 24, 32])
@pytest.mark.parametrize("S", [513, 640, 1000, 1024, 2048])
def test_long_slate_attention_matches_fp64(enc, S, dk, p):
    """Three slates: a padded tail, a full slate, a slate without any unmasked document (zeros, lse2 = +inf)."""
    h = _HEADS[dk]
    B = 3 if S <= 1024 else 2
    d, T, seed, sid = h * dk, B * S, 1234 + S, 24
    torch.manual_seed(S + 7 * dk)
    qkv16 = bits(rnd(T, 3 * d, scale=1.5))
    mask = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    mask[0, S - S // 3:] = 1
    mask[B - 1] = 1
    ctx, lse = _fwd("ltr_enc_attention_fwd_lse", qkv16, mask, B, S, h, dk, p, seed, sid)
    dctx16 = bits(rnd(T, d))
    dqkv = _bwd("ltr_enc_attention_bwd_lse", qkv16, ctx, dctx16, lse, mask, B, S, h, dk, p, seed, sid)
    e_ctx, e_g = _check_against_reference(enc, qkv16, mask, B, S, h, dk, p, seed, sid, ctx, lse, dqkv, dctx16)
    if S in (1024, 2048) and dk in (16, 17):
        ledger_record(f"tiled attention S={S} dk={dk} p={p}: ctx vs fp64", e_ctx, tol=1e-2, note="bf16 operands")
        ledger_record(f"tiled attention S={S} dk={dk} p={p}: worst dqkv vs fp64", e_g, tol=1.5e-2, note="bf16 operands")
    # the plain forward entry (no lse) runs the same kernel
    ctx0, _ = _fwd("ltr_enc_attention_fwd", qkv16, mask, B, S, h, dk, p, seed, sid, lse=False)
    assert torch.equal(ctx0, ctx)


@pytest.mark.parametrize("S,dk,p", [(513, 16, 0.1), (1000, 17, 0.0), (2048, 32, 0.1)])
def test_long_slate_attention_without_mask(enc, S, dk, p):
    h, B = _HEADS[dk], 2
    d, T, seed, sid = h * dk, B * S, 77, 3
    torch.manual_seed(S + dk)
    qkv16 = bits(rnd(T, 3 * d, scale=1.5))
    ctx, lse = _fwd("ltr_enc_attention_fwd_lse", qkv16, None, B, S, h, dk, p, seed, sid)
    dctx16 = bits(rnd(T, d))
    dqkv = _bwd("ltr_enc_attention_bwd_lse", qkv16, ctx, dctx16, lse, None, B, S, h, dk, p, seed, sid)
    _check_against_reference(enc, qkv16, None, B, S, h, dk, p, seed, sid, ctx, lse, dqkv, dctx16)


# ------------------------------------------------------------------------------------------------- 2. tiled vs whole-row
@pytest.mark.parametrize("S,dk,p", [(32, 16, 0.0), (100, 17, 0.1), (256, 16, 0.1), (300, 24, 0.0), (512, 32, 0.1), (512, 16, 0.0)])
def test_tiled_kernels_agree_with_the_whole_row_kernels(enc, S, dk, p):
    """ctx bar 8e-3 of its largest entry: the whole-row kernel rounds the NORMALISED (and dropout-scaled) probabilities to bf16 before
    P V, the tiled one the unnormalised p~ = 2^(c2 s - m) and divides by the sum afterwards -- two different bf16 rounding points of
    2^-9 relative each, after which both round ctx to bf16 (one ulp of the largest entry = 3.9e-3): two ulps cover both.  lse2
    differs only by the order of the fp32 sum (running rescales vs one pass): ~1e-6 relative.  dqkv: 1e-2."""
    h, B = _HEADS[dk] if dk != 16 else 4, 3
    d, T, seed, sid = h * dk, B * S, 555, 40
    torch.manual_seed(S * dk)
    qkv16 = bits(rnd(T, 3 * d, scale=1.5))
    mask = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    mask[1, S - S // 4:] = 1
    mask[2] = 1
    ctx_w, lse_w = _fwd("ltr_enc_attention_fwd_lse", qkv16, mask, B, S, h, dk, p, seed, sid)
    ctx_t, lse_t = _fwd("ltr_enc_attention_fwd_tiled", qkv16, mask, B, S, h, dk, p, seed, sid)
    e_ctx = err(unbits(ctx_t), unbits(ctx_w))
    assert e_ctx < 8e-3, e_ctx
    live = torch.isfinite(lse_w)
    assert torch.equal(live, torch.isfinite(lse_t)) and torch.all(lse_t[~live] > 0)
    e_lse = float(((lse_t[live] - lse_w[live]).abs() / lse_w[live].abs().clamp_min(1.0)).max())
    assert e_lse < 1e-6, e_lse
    dctx16 = bits(rnd(T, d))
    # the two backward kernels on the SAME forward outputs (ctx enters through D = dctx . ctx: fed each pair's own ctx, the
    # comparison would measure the forwards' rounding difference again -- 1.45e-2 of the largest dk entry at S = 32)
    g_w = _bwd("ltr_enc_attention_bwd_lse", qkv16, ctx_w, dctx16, lse_w, mask, B, S, h, dk, p, seed, sid)
    g_t = _bwd("ltr_enc_attention_bwd_tiled", qkv16, ctx_w, dctx16, lse_w, mask, B, S, h, dk, p, seed, sid)
    e_g = max(err(unbits(g_t)[:, j * d:(j + 1) * d], unbits(g_w)[:, j * d:(j + 1) * d]) for j in range(3))
    assert e_g < 1e-2, e_g
    # and the tiled pair end to end (its own forward's ctx and lse2) against fp64 at the bars of the long slates
    g_tt = _bwd("ltr_enc_attention_bwd_tiled", qkv16, ctx_t, dctx16, lse_t, mask, B, S, h, dk, p, seed, sid)
    _check_against_reference(enc, qkv16, mask, B, S, h, dk, p, seed, sid, ctx_t, lse_t, g_tt, dctx16)
    ledger_record(f"tiled vs whole-row attention S={S} dk={dk} p={p}: ctx", e_ctx, tol=8e-3,
                  note="different bf16 rounding point of P (normalised vs unnormalised)")
    ledger_record(f"tiled vs whole-row attention S={S} dk={dk} p={p}: lse2 (relative)", e_lse, tol=1e-6, note="fp32 sum order")
    ledger_record(f"tiled vs whole-row attention S={S} dk={dk} p={p}: worst dqkv", e_g, tol=1e-2, note="bf16 operands")


# ------------------------------------------------------------------------------------------------- 3. determinism
@pytest.mark.parametrize("S,dk,p", [(1000, 16, 0.1), (2048, 17, 0.1), (777, 24, 0.0)])
def test_long_slate_attention_is_bit_reproducible(enc, S, dk, p):
    h, B = _HEADS[dk] if dk != 16 else 8, 2
    d, T, seed, sid = h * dk, B * S, 9, 11
    torch.manual_seed(S)
    qkv16 = bits(rnd(T, 3 * d, scale=1.5))
    mask = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    mask[1, S // 2:] = 1
    dctx16 = bits(rnd(T, d))
    runs = []
    for _ in range(2):
        ctx, lse = _fwd("ltr_enc_attention_fwd_lse", qkv16, mask, B, S, h, dk, p, seed, sid)
        dqkv = _bwd("ltr_enc_attention_bwd_lse", qkv16, ctx, dctx16, lse, mask, B, S, h, dk, p, seed, sid)
        runs.append((ctx, lse, dqkv))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------- 4. p_attn
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_long_slate_probabilities(enc, p):
    lib, _ptr, _stream = _L()
    B, S, h, dk = 2, 1000, 4, 16
    d, T, seed, sid = h * dk, B * S, 31, 0
    torch.manual_seed(3)
    qkv16 = bits(rnd(T, 3 * d, scale=1.5))
    mask = torch.zeros(B, S, dtype=torch.uint8, device=DEV)
    mask[1, 700:] = 1
    probs = torch.empty(B, h, S, S, device=DEV)
    assert lib.ltr_enc_attention_probs(_ptr(qkv16), _ptr(mask), B, S, h, dk, p, seed, sid, _ptr(probs), _stream()) == 0
    q, k = (unbits(qkv16)[:, j * d:(j + 1) * d].view(B, S, h, dk).transpose(1, 2) for j in range(2))
    sc = (q @ k.transpose(-2, -1) / math.sqrt(dk)).masked_fill((mask == 1).view(B, 1, 1, S), float("-inf"))
    want = torch.softmax(sc, -1)
    if p:
        want = want * enc.attn_dropout_mask(seed, sid, B, S, h, p, DEV).double() / (1 - p)
    assert float((probs.double() - want).abs().max()) < 1e-4        # fp32 scores and exponent; probabilities <= 1 / (1 - p)
    if not p:
        assert float((probs.double().sum(-1) - 1).abs().max()) < 1e-4
    assert float(probs[1, :, :, 700:].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------- 5. whole network
# The gate of test_encoder_gpu._oracle_gate (the rounding-faithful oracle at bars derived from its own fp32-vs-fp64 deviation) with
# the long-slate exceptions named here instead of in tests/golden/encoder_noise_scaled.json (the older goldens' list, unchanged):
#   * _LONG_SINGLE_ENTRY: ONE entry of the kernels' gradient above the fixed max-norm bar while L2, cosine and norm ratio hold.
#     The oracle rounds the NORMALISED probabilities to bf16 (the whole-row kernels' rounding point); the tiled kernels round the
#     unnormalised p~ and divide afterwards, so single bf16 roundings of ctx differ and flip FFN ReLU gates downstream -- the
#     pattern of the FFN w_1 tensors of the S = 256 goldens (kernel max-norm up to 0.21 there).  Measured: 4.50e-2 / 4.87e-2.
#   * tensors whose self-test itself passes the fixed bars get the noise-scaled bars (max-norm 2x, L2 1.5x the self-noise).
_LONG_SINGLE_ENTRY = {"fc32_enc2_h4_S1000::encoder.layers.1.feed_forward.w_1.weight",
                      "fc32_enc2_h4_S1000::encoder.layers.1.feed_forward.w_1.bias"}


def _long_gate(got, scores, sd, x, mask, cfg, y, keep=None, what=""):
    import ltr_encoder_oracle as EO
    import ltr_oracle as O
    from test_encoder_gpu import _gerr, _l2err
    res = {dt: EO.scores_and_grads(sd, x.cpu(), mask.cpu(), cfg, lambda s_, dt=dt: O.approx_ndcg(s_, y.cpu().to(dt)), keep=keep, bf16=True,
                                   round_bwd=True, dtype=dt) for dt in (torch.float64, torch.float32)}
    s_o, _, g_o = res[torch.float64]
    e_s = relerr(scores.detach().cpu().numpy(), s_o.numpy())
    assert e_s < 1e-2, (what, "output", e_s)
    g_o = {k: v.double() for k, v in g_o.items()}
    g_n = {k: v.double() for k, v in res[torch.float32][2].items()}
    gmax = max(float(v.abs().max()) for v in g_o.values())
    out, bad = dict(max=0.0, noise_max=0.0, min_cos=1.0), []
    for k, want in g_o.items():
        g, n = got[k].double().reshape(want.shape), g_n[k]
        e_max, n_max, e_l2, n_l2 = _gerr(g, want, gmax), _gerr(n, want, gmax), _l2err(g, want, gmax), _l2err(n, want, gmax)
        single = f"{what}::{k}" in _LONG_SINGLE_ENTRY
        if single:
            ledger_record(f"{what}::{k} (single-entry bar)", e_max, noise=n_max, tol=6e-2, note="tiled P rounding point; L2 at the fixed bar")
        if e_max > (6e-2 if single else max(2e-2, 2 * n_max)):
            bad.append((k, "max-norm", e_max, "self-noise", n_max))
        if e_l2 > max(1.5e-2, 1.5 * n_l2):
            bad.append((k, "L2", e_l2, "self-noise", n_l2))
        if float(want.abs().max()) >= 0.05 * gmax:
            c = float(g.flatten() @ want.flatten() / max(float(g.norm() * want.norm()), 1e-300))
            cn = float(n.flatten() @ want.flatten() / max(float(n.norm() * want.norm()), 1e-300))
            r, rn = float(g.norm() / want.norm()), float(n.norm() / want.norm())
            if c < 1 - max(1e-3, 2 * (1 - cn)):
                bad.append((k, "cosine", c, "self", cn))
            if abs(r - 1) > max(2e-2, 2 * abs(rn - 1)):
                bad.append((k, "norm ratio", r, "self", rn))
            out["min_cos"] = min(out["min_cos"], c)
        if not single:
            out.update(max=max(out["max"], e_max), noise_max=max(out["noise_max"], n_max))
    assert not bad, (what, bad)
    return out


def _long_net(dropout, F=16):
    from architeture.multiLayer import make_model
    fc = dict(sizes=[32], input_norm=False, activation=None, dropout=0.0)
    tr = dict(N=2, d_ff=64, h=4, dropout=dropout, positional_encoding=None)
    return make_model(copy.deepcopy(fc), copy.deepcopy(tr), dict(d_output=1, output_activation=None), F).to(DEV), fc, tr


def test_long_slate_network_train_mode_matches_oracle_under_exported_masks(enc):
    import ltr_encoder_oracle as EO
    from losses.approxNDCG import approxNDCGLoss
    torch.manual_seed(8)
    F, B, S = 16, 2, 1000
    net, fc, tr = _long_net(0.1, F)
    net.train()
    x = torch.randn(B, S, F, device=DEV)
    y = torch.randint(0, 5, (B, S), device=DEV).float()
    mask = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    mask[1, 811:] = True
    y[mask] = -1
    net.ltr_seed = 91
    scores = net(x, mask, None)
    seed = (91 + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    approxNDCGLoss(scores, y).backward()
    T, d, dff, h = B * S, 32, 64, 4
    keep = {}
    for l in range(2):
        keep[("attn", l)] = enc.attn_dropout_mask(seed, enc.stream_attn(l), B, S, h, 0.1, DEV).cpu()
        keep[("attn_out", l)] = enc.dropout_mask(seed, enc.stream_attn_out(l), T * d, 0.1, DEV).view(T, d).cpu()
        keep[("ffn_hidden", l)] = enc.dropout_mask(seed, enc.stream_ffn_hidden(l), T * dff, 0.1, DEV).view(T, dff).cpu()
        keep[("ffn_out", l)] = enc.dropout_mask(seed, enc.stream_ffn_out(l), T * d, 0.1, DEV).view(T, d).cpu()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    cfg = EO.config_of(dict(fc_model=fc, transformer=tr), F)
    got = {k: p.grad.cpu().double() for k, p in net.named_parameters()}
    gate = _long_gate(got, scores, sd, x, mask, cfg, y, keep=keep, what="train-mode dropout S=1000")
    ledger_record("encoder S=1000 train-mode worst param-grad vs rounding-faithful oracle under exported masks (max-norm)", gate["max"],
                  noise=gate["noise_max"], tol=max(2e-2, 4 * gate["noise_max"]), note="bf16 bars, tests/test_encoder_gpu.py")


def _golden_long():
    with open(os.path.join(HERE, "golden", "manifest_r5.json")) as f:
        case = json.load(f)["encoder_long"][0]
    return case, np.load(os.path.join(HERE, "golden", "encoder_long.npz"), allow_pickle=False)


def test_long_slate_network_eval_vs_reference_golden():
    """Eval mode at S = 1000 against the reference (tests/golden/make_golden_r5.py): the rounding-faithful oracle gate (_long_gate) plus the reference's own fp32 scores / loss / gradients at the loose bars used there."""
    import ltr_encoder_oracle as EO
    from architeture.multiLayer import make_model
    from losses.approxNDCG import approxNDCGLoss
    from test_encoder_gpu import _gerr
    case, g = _golden_long()
    cid = case["id"]
    net = make_model(fc_model=copy.deepcopy(case["fc_model"]), transformer=copy.deepcopy(case["transformer"]),
                     post_model=dict(d_output=1, output_activation="Sigmoid"), n_features=case["n_features"])
    sd = {k: torch.from_numpy(g[f"{cid}/w/{k}"]) for k in case["keys"]}
    net.load_state_dict(sd)
    net = net.to(DEV).eval()
    x = torch.from_numpy(g[f"{cid}/x"]).to(DEV)
    y = torch.from_numpy(g[f"{cid}/y"]).to(DEV)
    mask = torch.from_numpy(g[f"{cid}/mask"]).to(DEV)
    assert x.shape[1] == 1000 and bool(mask.any())
    scores = net(x, mask, None)
    loss = approxNDCGLoss(scores, y)
    loss.backward()
    got = {k: p.grad.cpu().double() for k, p in net.named_parameters()}
    cfg = EO.config_of(dict(fc_model=case["fc_model"], transformer=case["transformer"]), case["n_features"])
    gate = _long_gate(got, scores, sd, x, mask, cfg, y, what=cid)
    want_s = g[f"{cid}/scores"]
    assert relerr(scores.detach().cpu().numpy(), want_s) < 3e-2
    assert abs(float(loss) - float(g[f"{cid}/loss"])) < 3e-2 * abs(float(g[f"{cid}/loss"]))
    ref = {k: torch.from_numpy(g[f"{cid}/g/{k}"]).double() for k in case["keys"]}
    flat_got, flat_ref = torch.cat([got[k].flatten() for k in ref]), torch.cat([ref[k].flatten() for k in ref])
    cos = float(flat_got @ flat_ref / (flat_got.norm() * flat_ref.norm()))
    assert cos > 0.99, cos
    gmax = max(float(v.abs().max()) for v in ref.values())
    ledger_record("encoder S=1000 worst param-grad vs rounding-faithful oracle (max-norm)", gate["max"], noise=gate["noise_max"],
                  tol=max(2e-2, 4 * gate["noise_max"]), note=f"min cosine {gate['min_cos']:.6f}")
    ledger_record("encoder S=1000 worst param-grad vs reference fp32 (ledger only, not a gate)",
                  max(_gerr(got[k], ref[k], gmax) for k in ref), tol=1.0, asserted=False, note=f"whole-gradient cosine {cos:.5f}")


# ------------------------------------------------------------------------------------------------- 6. standalone blocks
def _ln64(x, a, b, eps=1e-6):
    return a * (x - x.mean(-1, keepdim=True)) / (x.std(-1, keepdim=True) + eps) + b


def _mha64(sd, pre, x, mask, h):
    B, S, d = x.shape
    dk = d // h
    lin = lambda i, t: t @ sd[f"{pre}linears.{i}.weight"].T + sd[f"{pre}linears.{i}.bias"]      # noqa: E731
    q, k, v = (lin(i, x).view(B, S, h, dk).transpose(1, 2) for i in range(3))
    sc = (q @ k.transpose(-2, -1) / math.sqrt(dk)).masked_fill(mask.view(B, 1, 1, S), float("-inf"))
    return lin(3, (torch.softmax(sc, -1) @ v).transpose(1, 2).reshape(B, S, d))


def _grad_err(got, want):
    gmax = max(float(w.abs().max()) for w in want.values())
    return max(float((got[k] - w).abs().max()) / max(float(w.abs().max()), 0.05 * gmax) for k, w in want.items())


def test_long_slate_standalone_blocks():
    """attention() (output and p_attn), MultiHeadedAttention and EncoderLayer at S = 768 with gradients, against fp64 restatements
    of transformer.py on the device (same weights), at the bars of tests/test_blocks_gpu.py (output 2e-2 / 3e-2 composite,
    gradients 4e-2 for the one-GEMM blocks, whole-gradient cosine 0.99 for EncoderLayer)."""
    from architeture import transformer as T
    torch.manual_seed(21)
    B, S, h, d, dff = 2, 768, 4, 64, 128
    pad = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    pad[1, 600:] = True
    # attention()
    q, k, v = (torch.randn(B, h, S, d // h, device=DEV, requires_grad=True) for _ in range(3))
    out, p_attn = T.attention(q, k, v, mask=pad.view(B, 1, 1, S).to(torch.uint8), dropout=None)
    q64, k64, v64 = (t.detach().double().requires_grad_(True) for t in (q, k, v))
    sc = (q64 @ k64.transpose(-2, -1) / math.sqrt(d // h)).masked_fill(pad.view(B, 1, 1, S), float("-inf"))
    pa = torch.softmax(sc, -1)
    want = pa @ v64
    assert err(out.detach(), want.detach()) < 2e-2
    assert tuple(p_attn.shape) == (B, h, S, S) and err(p_attn, pa.detach()) < 1e-2
    w = torch.randn_like(want)
    (out * w.float()).sum().backward()
    (want * w).sum().backward()
    assert _grad_err({n: t.grad.double() for n, t in zip("qkv", (q, k, v))}, {n: t.grad for n, t in zip("qkv", (q64, k64, v64))}) < 4e-2
    # MultiHeadedAttention and EncoderLayer
    for kind in ("MultiHeadedAttention", "EncoderLayer"):
        if kind == "MultiHeadedAttention":
            mod = T.MultiHeadedAttention(h, d, 0.1)
        else:
            mod = T.EncoderLayer(d, T.MultiHeadedAttention(h, d, 0.1), T.PositionwiseFeedForward(d, dff, 0.1), 0.1)
        with torch.no_grad():
            for prm in mod.parameters():
                if prm.dim() == 1:
                    prm.add_(0.1 * torch.randn_like(prm))
        mod = mod.to(DEV).eval()
        x = torch.randn(B, S, d, device=DEV, requires_grad=True)
        m3 = pad.view(B, 1, S)
        out = mod(x, x, x, m3) if kind == "MultiHeadedAttention" else mod(x, m3)
        sd = {n: t.detach().double().requires_grad_(True) for n, t in mod.named_parameters()}
        x64 = x.detach().double().requires_grad_(True)
        if kind == "MultiHeadedAttention":
            want = _mha64(sd, "", x64, pad, h)
        else:
            x1 = x64 + _mha64(sd, "self_attn.", _ln64(x64, sd["sublayer.0.norm.a_2"], sd["sublayer.0.norm.b_2"]), pad, h)
            n2 = _ln64(x1, sd["sublayer.1.norm.a_2"], sd["sublayer.1.norm.b_2"])
            hid = torch.relu(n2 @ sd["feed_forward.w_1.weight"].T + sd["feed_forward.w_1.bias"])
            want = x1 + hid @ sd["feed_forward.w_2.weight"].T + sd["feed_forward.w_2.bias"]
        e_out = err(out.detach(), want.detach())
        assert e_out < (2e-2 if kind == "MultiHeadedAttention" else 3e-2), (kind, e_out)
        w = torch.randn_like(want)
        (out * w.float()).sum().backward()
        (want * w).sum().backward()
        got = {n: t.grad.double() for n, t in mod.named_parameters()}
        got["x"] = x.grad.double()
        ref = {n: t.grad for n, t in sd.items()}
        ref["x"] = x64.grad
        e_g = _grad_err(got, ref)
        if kind == "MultiHeadedAttention":
            assert e_g < 4e-2, (kind, e_g)
        else:       # a composite block (tests/test_blocks_gpu.py): whole-gradient cosine; single FFN entries flip ReLU gates vs fp64
            fg, fr = torch.cat([got[n].flatten() for n in ref]), torch.cat([ref[n].flatten() for n in ref])
            cos = float(fg @ fr / (fg.norm() * fr.norm()))
            assert cos > 0.99, (kind, cos)
            ledger_record("EncoderLayer S=768 worst gradient vs fp64 (ledger only, not a gate)", e_g, tol=1.0, asserted=False,
                          note=f"whole-gradient cosine {cos:.6f}")


# ------------------------------------------------------------------------------------------------- 7. graphed step
def test_graphed_long_slate_step_equals_eager_steps(enc, monkeypatch):
    from architeture.multiLayer import LTRModel, make_model
    from losses.approxNDCG import approxNDCGLoss
    from ltr_mi355x import blocks
    from ltr_mi355x.graphs import GraphedTrainStep
    SEED = 0x0DDBA11CAFEF00D
    monkeypatch.setattr(blocks, "fresh_seed", lambda: SEED)
    monkeypatch.setattr(LTRModel, "_ltr_next_seed", lambda self: SEED)
    B, S, F = 4, 1024, 136
    gen = torch.Generator(device=DEV).manual_seed(4)
    x = torch.randn(B, S, F, device=DEV, generator=gen)
    y = torch.randint(0, 5, (B, S), device=DEV, generator=gen).float()
    mask = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    mask[2, 900:] = True
    y[2, 900:] = -1.0

    def loss_fn(net, x, mask, y):
        return approxNDCGLoss(net(x, mask, None), y)
    torch.manual_seed(3)
    net_g = make_model(dict(sizes=[128], input_norm=False, activation=None, dropout=0.1),
                       dict(N=2, d_ff=256, h=8, dropout=0.1, positional_encoding=None), dict(d_output=1, output_activation=None), F).to(DEV).train()
    net_e = copy.deepcopy(net_g)
    opt_g = torch.optim.Adam(net_g.parameters(), lr=1e-3, capturable=True)
    opt_e = torch.optim.Adam(net_e.parameters(), lr=1e-3, capturable=True)
    E0 = 500
    try:
        enc.seed_set(E0)
        step = GraphedTrainStep(net_g, opt_g, loss_fn, (x, mask, y), warmup=2)
        losses_g = [float(step(x, mask, y).detach()) for _ in range(2)]
        assert enc.seed_get() == E0 + 4
        losses_e = []
        for k in range(1, 5):
            enc.seed_set(E0 + k)
            opt_e.zero_grad(set_to_none=True)
            l = loss_fn(net_e, x, mask, y)
            l.backward()
            opt_e.step()
            losses_e.append(float(l.detach()))
        assert losses_g == losses_e[2:]
        for (n, a), b in zip(net_g.named_parameters(), net_e.parameters()):
            assert torch.equal(a, b), n
    finally:
        enc.seed_set(0)
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- 8. limits
def test_long_slate_limits(enc):
    from ltr_mi355x._lib import lib as _lib
    from ltr_mi355x.functional import _ptr, _stream
    lib = _lib()
    SHAPE = -2                                   # LTR_ERR_SHAPE, include/ltr_mi355x.h
    B, h, dk = 1, 2, 16
    d = h * dk
    for S in (2049, 4096):
        qkv = torch.zeros(B * S, 3 * d, dtype=torch.int16, device=DEV)
        out = torch.zeros(B * S, 3 * d, dtype=torch.int16, device=DEV)
        lse = torch.zeros(B * h, S, device=DEV)
        for name, rc in (("fwd", lib.ltr_enc_attention_fwd(_ptr(qkv), None, B, S, h, dk, 0.0, 0, 0, _ptr(out), _stream())),
                         ("fwd_lse", lib.ltr_enc_attention_fwd_lse(_ptr(qkv), None, B, S, h, dk, 0.0, 0, 0, _ptr(out), _ptr(lse), _stream())),
                         ("fwd_tiled", lib.ltr_enc_attention_fwd_tiled(_ptr(qkv), None, B, S, h, dk, 0.0, 0, 0, _ptr(out), _ptr(lse), _stream())),
                         ("bwd_lse", lib.ltr_enc_attention_bwd_lse(_ptr(qkv), _ptr(out), _ptr(out), _ptr(lse), None, B, S, h, dk, 0.0, 0, 0,
                                                                   _ptr(out), _stream())),
                         ("bwd_tiled", lib.ltr_enc_attention_bwd_tiled(_ptr(qkv), _ptr(out), _ptr(out), _ptr(lse), None, B, S, h, dk, 0.0, 0, 0,
                                                                       _ptr(out), _stream())),
                         ("probs", lib.ltr_enc_attention_probs(_ptr(qkv), None, B, S, h, dk, 0.0, 0, 0, _ptr(lse), _stream()))):
            assert rc == SHAPE, (name, S, rc)
    # without the forward's row statistics the backward stops at 512; the tiled entries require them
    for S, want in ((512, 0), (513, SHAPE), (2048, SHAPE)):
        qkv = torch.zeros(B * S, 3 * d, dtype=torch.int16, device=DEV)
        ctx = torch.zeros(B * S, d, dtype=torch.int16, device=DEV)
        out = torch.zeros(B * S, 3 * d, dtype=torch.int16, device=DEV)
        assert lib.ltr_enc_attention_bwd(_ptr(qkv), _ptr(ctx), _ptr(ctx), None, B, S, h, dk, 0.0, 0, 0, _ptr(out), _stream()) == want
        assert lib.ltr_enc_attention_bwd_lse(_ptr(qkv), _ptr(ctx), _ptr(ctx), None, None, B, S, h, dk, 0.0, 0, 0, _ptr(out), _stream()) == want
        assert lib.ltr_enc_attention_bwd_tiled(_ptr(qkv), _ptr(ctx), _ptr(ctx), None, None, B, S, h, dk, 0.0, 0, 0, _ptr(out), _stream()) != 0
        assert lib.ltr_enc_attention_fwd_tiled(_ptr(qkv), None, B, S, h, dk, 0.0, 0, 0, _ptr(ctx), None, _stream()) != 0
    torch.cuda.synchronize()
    # Python: 2048 documents run, 2049 raise and name the limit
    net, _, _ = _long_net(0.0, 8)
    net.eval()
    with torch.no_grad():
        assert net(torch.randn(1, 2048, 8, device=DEV), torch.zeros(1, 2048, dtype=torch.bool, device=DEV), None).shape == (1, 2048)
        with pytest.raises(ValueError, match="2048"):
            net(torch.randn(1, 2049, 8, device=DEV), torch.zeros(1, 2049, dtype=torch.bool, device=DEV), None)
