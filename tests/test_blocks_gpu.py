"""GPU parity of the building blocks of architeture/transformer.py / multiLayer.py called ON THEIR OWN
against goldens produced by the REAL reference modules (tests/golden/make_golden_r4.py -> blocks.npz: eval mode, fp32 CPU):
output, gradient w.r.t. every parameter and w.r.t. the input of  sum(out * w_out).

Arithmetic of the HIP path: bf16 operands on the matrix cores, fp32 accumulation -- so the bars are bf16 bars, stated here:
  * LayerNorm and OutputLayer(d_output = 1) are fp32 throughout: 2e-5 vs the reference module.
  * one- and two-GEMM blocks (Linear / OutputLayer d_output = 3, FCModel, PositionwiseFeedForward, MultiHeadedAttention,
    attention(), SublayerConnection): output within 2e-2 of its max, every gradient within 4e-2 (max-norm, on max(its own
    scale, 5 % of the case's largest gradient entry)), direction cos > 0.999 where it is not noise -- vs the reference module.
  * composite blocks (EncoderLayer, Encoder, LTRModel with d_output = 3, prepare_for_output): vs the reference module the
    bf16 operand rounding of 5-10 chained GEMMs in a 32-wide network is 0.08-0.15 per tensor (recorded, sanity-checked:
    output 3e-2, whole-gradient cosine > 0.99); the GATE is the rounding-faithful fp64 oracle (oracle/ltr_encoder_oracle.py,
    pinned on these very blocks against the reference at 2e-5 in fp32) at the measured-noise bars of tests/test_encoder_gpu.py.
Observed values go to the parity ledger."""
import numpy as np
import pytest
import torch

from conftest import golden, ledger_record, relerr
from test_encoder_gpu import _oracle_gate

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _build(case):
    from architeture import transformer as T
    from architeture.multiLayer import FCModel, OutputLayer, make_model
    import copy
    k = case["kind"]
    if k == "LayerNorm":
        return T.LayerNorm(case["d"])
    if k == "PositionwiseFeedForward":
        return T.PositionwiseFeedForward(case["d"], case["d_ff"], 0.1)
    if k == "MultiHeadedAttention":
        return T.MultiHeadedAttention(case["h"], case["d"], 0.1)
    if k == "SublayerConnection":
        return T.SublayerConnection(case["d"], 0.1)
    if k == "EncoderLayer":
        return T.EncoderLayer(case["d"], T.MultiHeadedAttention(case["h"], case["d"], 0.1), T.PositionwiseFeedForward(case["d"], case["d_ff"], 0.1), 0.1)
    if k == "Encoder":
        return T.make_transformer(N=case["N"], d_ff=case["d_ff"], h=case["h"], dropout=0.1, n_features=case["d"])
    if k == "FCModel":
        return FCModel(sizes=copy.deepcopy(case["sizes"]), input_norm=case["input_norm"], activation=None, dropout=0.2 if case["input_norm"] else 0.0,
                       n_features=case["n_features"])
    if k == "OutputLayer":
        return OutputLayer(case["d"], case["d_output"], None)
    if k == "LTRModel":
        return make_model(dict(sizes=[case["d"]], input_norm=False, activation=None, dropout=0.0),
                          dict(N=case["N"], d_ff=case["d_ff"], h=case["h"], dropout=0.0, positional_encoding=None),
                          dict(d_output=case["d_output"], output_activation=None), case["n_features"])
    return None


def _call(case, mod, ins, g):
    from architeture import transformer as T
    k = case["kind"]
    if k in ("LayerNorm", "PositionwiseFeedForward", "FCModel"):
        return mod(ins[0])
    if k == "MultiHeadedAttention":
        return mod(ins[0], ins[0], ins[0], ins[1]) if case["self_attn"] else mod(ins[0], ins[1], ins[2], ins[3])
    if k == "attention":
        return T.attention(ins[0], ins[1], ins[2], mask=ins[3], dropout=None)
    if k == "SublayerConnection":
        ff = T.PositionwiseFeedForward(case["d"], case["d_ff"], 0.1)
        gff = golden("blocks")
        ffc = next(c for c in gff.cases if c["id"] == "PositionwiseFeedForward")
        ff.load_state_dict({kk: torch.from_numpy(gff.arr(ffc, "w/" + kk)) for kk in ffc["keys"]})
        ff = ff.to(DEV).eval()
        for p in ff.parameters():
            p.requires_grad_(False)
        return mod(ins[0], ff)
    if k == "EncoderLayer":
        return mod(ins[0], ins[1])
    if k == "Encoder":
        return mod(ins[0], ins[1], None)
    if k == "OutputLayer":
        return mod(ins[0]) if case["method"] == "forward" else mod.score(ins[0])
    if k == "LTRModel":
        return getattr(mod, case["method"])(ins[0], ins[1], None)
    raise AssertionError(k)


@pytest.mark.parametrize("case", golden("blocks").cases, ids=lambda c: c["id"])
def test_block_on_its_own_matches_the_reference_module(case):
    g = golden("blocks")
    mod = _build(case)
    if mod is not None:
        assert list(mod.state_dict().keys()) == case["keys"]
        mod.load_state_dict({k: torch.from_numpy(g.arr(case, "w/" + k)) for k in case["keys"]})
        mod = mod.to(DEV).eval()
    ins = []
    for i in range(case["n_inputs"]):
        t = torch.from_numpy(g.arr(case, f"in{i}")).to(DEV)
        ins.append(t.requires_grad_(True) if t.is_floating_point() else t)
    out = _call(case, mod, ins, g)
    out1 = None
    if isinstance(out, tuple):
        out, out1 = out
    want = g.arr(case, "out")
    assert tuple(out.shape) == want.shape
    exact = case["kind"] == "LayerNorm" or (case["kind"] == "OutputLayer" and case["d_output"] == 1)
    composite = case["kind"] in ("EncoderLayer", "Encoder", "LTRModel")
    tol_o, tol_g = (2e-5, 2e-5) if exact else ((3e-2, None) if composite else (2e-2, 4e-2))
    e_out = relerr(out.detach().cpu().numpy(), want)
    assert e_out < tol_o, e_out
    if out1 is not None:                                     # attention(): p_attn
        assert relerr(out1.cpu().numpy(), g.arr(case, "out1")) < 1e-2
    w_out = torch.from_numpy(g.arr(case, "w_out"))
    (out * w_out.to(DEV)).sum().backward()
    pairs = {}
    for i, t in enumerate(ins):
        if t.is_floating_point():
            assert t.grad is not None, f"no gradient w.r.t. input {i}"
            pairs[f"din{i}"] = (t.grad.cpu().double(), torch.from_numpy(g.arr(case, f"din{i}")).double())
    if mod is not None:
        for k, p in mod.named_parameters():
            ref = torch.from_numpy(g.arr(case, "g/" + k)).double()
            got = torch.zeros_like(ref) if p.grad is None else p.grad.cpu().double()
            pairs["g/" + k] = (got, ref)
    gmax = max(float(r.abs().max()) for _, r in pairs.values())
    worst, worst_cos = 0.0, 1.0
    for k, (got, ref) in pairs.items():
        scale = max(float(ref.abs().max()), 0.05 * gmax)
        e = float((got - ref).abs().max()) / scale
        worst = max(worst, e)
        if float(ref.abs().max()) >= 0.05 * gmax:
            worst_cos = min(worst_cos, float(got.flatten() @ ref.flatten() / (got.norm() * ref.norm())))
        if not composite:
            assert e < tol_g, (k, e)
    note = "standalone block vs the reference module (fp32 CPU); bf16-operand arithmetic: bars stated in tests/test_blocks_gpu.py"
    if composite:
        fg, fr = torch.cat([a_.flatten() for a_, _ in pairs.values()]), torch.cat([b_.flatten() for _, b_ in pairs.values()])
        assert float(fg @ fr / (fg.norm() * fr.norm())) > 0.99
        gate = _composite_gate(case, g, mod, ins, out, pairs, w_out)
        ledger_record(f"block {case['id']} worst gradient vs rounding-faithful oracle (max-norm)", gate["max"], noise=gate["noise_max"],
                      tol=max(2e-2, 4 * gate["noise_max"]), note=note + f"; min cosine {gate['min_cos']:.6f}")
        ledger_record(f"block {case['id']} worst gradient vs the reference module (ledger only, not a gate)", worst, tol=1.0, note=note, asserted=False)
    else:
        assert worst_cos > 0.999, worst_cos
        ledger_record(f"block {case['id']} worst gradient (max-norm)", worst, tol=tol_g, note=note + f"; min cosine {worst_cos:.6f}")
    ledger_record(f"block {case['id']} output", e_out, tol=tol_o, note=note)


def _composite_gate(case, g, mod, ins, out, pairs, w_out):
    """EncoderLayer / Encoder / LTRModel(d_output = 3) through the oracle: its state_dict keys are LTRModel's."""
    k = case["kind"]
    prefix = {"EncoderLayer": "encoder.layers.0.", "Encoder": "encoder.", "LTRModel": ""}[k]
    sd = {prefix + kk: torch.from_numpy(g.arr(case, "w/" + kk)) for kk in case["keys"]}
    cfg = dict(n_fc=1 if k == "LTRModel" else 0, input_norm=False, fc_dropout=0.0, has_encoder=True, heads=case["h"], enc_dropout=0.0,
               n_layers=case.get("N", 1), final_norm=k != "EncoderLayer",
               output="scores" if (k == "LTRModel" and case["method"] != "prepare_for_output") else "features")
    x = torch.from_numpy(g.arr(case, "in0"))
    mask = torch.from_numpy(g.arr(case, "in1")).reshape(x.shape[0], x.shape[1])
    score_sum = k == "LTRModel" and case["method"] == "score"       # OutputLayer.score: the d_output outputs summed

    def loss_fn(o, dt):
        o = o.sum(-1) if score_sum else o
        return (o * w_out.to(dt)).sum()

    got = {prefix + kk[2:]: v[0] for kk, v in pairs.items() if kk.startswith("g/")}
    got["__x__"] = pairs["din0"][0]

    return _oracle_gate(got, out, sd, x, mask, cfg, None, what=case["id"], loss_fn=loss_fn, want_dx=True,
                        out_post=(lambda o: o.sum(-1)) if score_sum else None)


def test_blocks_train_mode_and_errors():
    """Dropout sites are live in train mode (outputs change between calls, eval is deterministic); attention shapes outside the fused
    kernels' run the reference's formulation on the device; CPU tensors raise."""
    from architeture import transformer as T
    torch.manual_seed(0)
    x = torch.randn(2, 16, 32, device=DEV)
    mask = torch.zeros(2, 16, dtype=torch.bool, device=DEV)
    enc = T.make_transformer(N=1, d_ff=64, h=4, dropout=0.3, n_features=32).to(DEV)
    enc.train()
    a, b = enc(x, mask, None), enc(x, mask, None)
    assert not torch.equal(a, b)
    enc.eval()
    assert torch.equal(enc(x, mask, None), enc(x, mask, None))
    with pytest.raises(AttributeError):
        enc(x, None, None)                                        # transformer.py:55 dereferences the mask
    # key / value sets unlike the query set and masks that are not one flag per document (transformer.py:145-164, :187-212 take them;
    # the reference's own callers never pass either): the reference's formulation on the device -- checked against the same
    # lines restated in fp64 on the CPU, values and gradients
    import math
    mha = T.MultiHeadedAttention(4, 32, 0.0).to(DEV).eval()

    def ref_mha(q, k, v, m):
        W = [(l.weight.detach().double().cpu(), l.bias.detach().double().cpu()) for l in mha.linears]
        nb = q.shape[0]
        qq, kk, vv = [(t @ w.T + b).view(nb, -1, 4, 8).transpose(1, 2) for t, (w, b) in zip((q, k, v), W[:3])]
        sc = qq @ kk.transpose(-2, -1) / math.sqrt(8)
        if m is not None:
            sc = sc.masked_fill(m.unsqueeze(1) == 1, float("-inf"))
        o = (torch.softmax(sc, -1) @ vv).transpose(1, 2).contiguous().view(nb, -1, 32)
        return o @ W[3][0].T + W[3][1]
    pq = torch.zeros(2, 16, 16, device=DEV)
    pq[:, :, 12:] = 1                                          # a [batch, query, key] mask
    for k_in, m in ((x, pq), (x[:, :8], None)):
        xq = x.clone().requires_grad_(True)
        out = mha(xq, k_in, k_in, m)
        out.square().sum().backward()
        xr = x.detach().double().cpu().requires_grad_(True)
        ref = ref_mha(xr, k_in.detach().double().cpu(), k_in.detach().double().cpu(), None if m is None else m.cpu())
        ref.square().sum().backward()
        assert relerr(out.detach().cpu().numpy(), ref.detach().numpy()) < 2e-5
        assert relerr(xq.grad.cpu().numpy(), xr.grad.numpy()) < 2e-5
    o2, p2 = T.attention(torch.randn(2, 4, 16, 8, device=DEV), torch.randn(2, 4, 5, 8, device=DEV), torch.randn(2, 4, 5, 8, device=DEV))
    assert tuple(o2.shape) == (2, 4, 16, 8) and tuple(p2.shape) == (2, 4, 16, 5)
    from ltr_mi355x._lib import LtrDeviceError as _DevErr
    with pytest.raises(_DevErr):
        T.attention(torch.randn(2, 4, 16, 8), torch.randn(2, 4, 5, 8), torch.randn(2, 4, 5, 8))      # no CPU path here either
    from ltr_mi355x._lib import LtrDeviceError
    with pytest.raises(LtrDeviceError):
        T.LayerNorm(32)(x.cpu())
    ff = T.PositionwiseFeedForward(32, 64, 0.5).to(DEV).train()
    assert not torch.equal(ff(x), ff(x))


def test_encoder_layer_with_mixed_dropout_probabilities_takes_the_composed_path():
    """An EncoderLayer whose four dropout modules carry DIFFERENT probabilities (attention, FFN hidden, the two residual
    sublayers; the reference applies each module's own p, transformer.py:106-142) must not run the fused node with one p: it
    walks the composed per-block path.  In eval mode (no dropout active) both paths compute the same function; in training
    mode the composed path's outputs differ between two calls only through dropout -- and with every p = 0 they are identical."""
    from architeture import transformer as T
    torch.manual_seed(3)
    d, h, dff = 64, 4, 128
    mixed = T.EncoderLayer(d, T.MultiHeadedAttention(h, d, 0.3), T.PositionwiseFeedForward(d, dff, 0.05), 0.2).to(DEV)
    mixed.sublayer[1].dropout.p = 0.4
    uniform = T.EncoderLayer(d, T.MultiHeadedAttention(h, d, 0.1), T.PositionwiseFeedForward(d, dff, 0.1), 0.1).to(DEV)
    uniform.load_state_dict(mixed.state_dict())
    x = torch.randn(3, 40, d, device=DEV)
    mask = torch.zeros(3, 40, dtype=torch.bool, device=DEV)
    mask[1, 30:] = True
    mixed.eval(), uniform.eval()
    a, b = mixed(x, mask), uniform(x, mask)
    assert relerr(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < 2e-2            # bf16 operands on both paths
    mixed.train()
    xg = x.clone().requires_grad_(True)
    out = mixed(xg, mask)
    out.square().mean().backward()
    assert torch.isfinite(out).all() and torch.isfinite(xg.grad).all()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mixed.parameters())
    # the fused node hands out a COPY of its residual stream (kept in ctx for the backward): editing the output's storage behind
    # autograd's back must not reach what the backward reads
    uniform.train(False)
    xg2 = x.clone().requires_grad_(True)
    o2 = uniform(xg2, mask)
    ref = torch.autograd.grad(o2.sum(), xg2, retain_graph=True)[0].clone()
    o2.data.zero_()
    again = torch.autograd.grad(o2.sum(), xg2)[0]
    assert torch.equal(ref, again)


class GemmLog:
    """encoder.gemm, encoder.splitk_epilogue and encoder._drop_cast_colsum wrapped for one call of a stand-alone block (in the spirit of
    test_encoder_gpu.FfnCalls): what every GEMM was asked for.  The blocks share their launch chains with the fused network
    (ltr_mi355x.encoder: attention_sublayer_*, ffn_gemm_*); these records pin what the network adds around a sublayer and a block on
    its own must not get -- residual, output dropout, split-K."""

    def __init__(self, monkeypatch):
        from ltr_mi355x import encoder as enc
        self.gemms, self.epilogues, self.grad_drops = [], [], []
        gemm, epilogue, drop_cast = enc.gemm, enc.splitk_epilogue, enc._drop_cast_colsum

        def logging_gemm(A, B, M, N, K, **kw):
            self.gemms.append(dict(shape=(M, N, K), a_kmajor=bool(kw.get("a_kmajor")), b_kmajor=bool(kw.get("b_kmajor")),
                                   drop_p=float(kw.get("drop_p", 0.0)), drop_stream=int(kw.get("drop_stream", 0)),
                                   residual=kw.get("residual") is not None, bias=kw.get("bias") is not None, splits=int(kw.get("splits", 1)),
                                   relu=bool(kw.get("relu")), gate=kw.get("gate") is not None, ldc=kw.get("ldc"),
                                   Cf=kw.get("Cf") is not None, Cb=kw.get("Cb") is not None))
            return gemm(A, B, M, N, K, **kw)

        def logging_epilogue(*args):
            self.epilogues.append(args)
            return epilogue(*args)

        def logging_drop_cast(dx, T, N, p, seed, stream_id):
            self.grad_drops.append((T, N, float(p)))
            return drop_cast(dx, T, N, p, seed, stream_id)

        monkeypatch.setattr(enc, "gemm", logging_gemm)
        monkeypatch.setattr(enc, "splitk_epilogue", logging_epilogue)
        monkeypatch.setattr(enc, "_drop_cast_colsum", logging_drop_cast)

    def forward_gemms(self, shape):
        """The row-major x row-major (activation x weight) GEMMs of that (M, N, K)."""
        return [g for g in self.gemms if g["shape"] == shape and not g["a_kmajor"] and not g["b_kmajor"]]


def test_feed_forward_on_its_own_never_splits_k_and_has_no_sublayer_epilogue(monkeypatch):
    """PositionwiseFeedForward(32, 1024) on 51 tokens: the fused network runs this shape's two (T, d, d_ff) GEMMs as 2 split-K slices
    with the residual and SublayerConnection's dropout in the reduce; the module on its own is w_2(dropout(relu(w_1 x))) and nothing else
    (transformer.py:231-237) -- one slice, no split-K epilogue, no residual, no dropout on the output, the module's p on the hidden layer."""
    from architeture import transformer as T
    from ltr_mi355x import encoder as enc
    tokens, d, dff = 51, 32, 1024
    assert enc._small_step_splits(tokens, d, dff) == 2
    torch.manual_seed(5)
    ff = T.PositionwiseFeedForward(d, dff).to(DEV).train()
    x = torch.randn(3, 17, d, device=DEV, requires_grad=True)
    log = GemmLog(monkeypatch)
    ff(x).square().sum().backward()
    assert x.grad is not None and torch.isfinite(x.grad).all()
    assert log.epilogues == []
    (hidden,) = [g for g in log.gemms if g["relu"]]
    assert hidden["shape"] == (tokens, dff, d) and hidden["bias"] and hidden["Cb"] and not hidden["residual"]
    assert hidden["drop_p"] == pytest.approx(ff.dropout.p) and ff.dropout.p > 0 and hidden["drop_stream"] == 2
    (out,) = log.forward_gemms((tokens, d, dff))
    assert out["splits"] == 1 and out["Cf"] and out["bias"] and not out["residual"] and out["drop_p"] == 0.0
    (dx,) = [g for g in log.gemms if g["shape"] == (tokens, d, dff) and g["b_kmajor"] and not g["a_kmajor"]]
    assert dx["splits"] == 1 and dx["Cf"] and not dx["gate"]
    assert log.grad_drops == [(tokens, d, 0.0)]              # the incoming gradient passes no output dropout


def test_multi_head_attention_on_its_own_projects_without_residual_or_output_dropout(monkeypatch):
    """MultiHeadedAttention(4, 32, 0.1) in train mode: its dropout is the one on the attention probabilities (transformer.py:207);
    the output projection carries neither a residual nor a dropout (those are SublayerConnection's, which the fused network folds
    into this GEMM).  query is key is value: ONE (T, 3d, d) projection GEMM; three distinct tensors: three (T, d, d) GEMMs into the
    column blocks of the packed [T, 3d] tensor (ldc = 3d)."""
    from architeture import transformer as T
    torch.manual_seed(6)
    B_, S, d = 3, 17, 32
    tokens = B_ * S
    mha = T.MultiHeadedAttention(4, d, 0.1).to(DEV).train()
    q, k, v = (torch.randn(B_, S, d, device=DEV, requires_grad=True) for _ in range(3))
    mask = torch.zeros(B_, 1, S, dtype=torch.bool, device=DEV)
    mask[1, :, 12:] = True
    log = GemmLog(monkeypatch)
    out = mha(q, q, q, mask)
    assert torch.isfinite(out).all()
    (qkv,) = log.forward_gemms((tokens, 3 * d, d))
    assert qkv["Cb"] and qkv["bias"] and qkv["ldc"] in (None, 3 * d)
    (proj,) = log.forward_gemms((tokens, d, d))
    assert proj["Cf"] and proj["bias"] and not proj["residual"] and proj["drop_p"] == 0.0
    assert len(log.gemms) == 2
    _backward_has_no_output_dropout(log, out, tokens, d)
    out = mha(q, k, v, mask)
    assert torch.isfinite(out).all()
    assert log.forward_gemms((tokens, 3 * d, d)) == []
    square = log.forward_gemms((tokens, d, d))
    packed, (proj,) = [g for g in square if g["Cb"]], [g for g in square if g["Cf"]]
    assert len(packed) == 3 and all(g["ldc"] == 3 * d and g["bias"] for g in packed)
    assert proj["bias"] and not proj["residual"] and proj["drop_p"] == 0.0
    assert len(log.gemms) == 4
    _backward_has_no_output_dropout(log, out, tokens, d)
    assert all(t.grad is not None and torch.isfinite(t.grad).all() for t in (q, k, v))


def _backward_has_no_output_dropout(log, out, tokens, d):
    """The backward of a stand-alone MultiHeadedAttention: the incoming gradient is cast with p = 0 (no SublayerConnection dropout to
    undo) and goes through Wo into the bf16 d ctx with a plain GEMM.  Clears the log."""
    log.gemms.clear()
    out.square().sum().backward()
    assert log.grad_drops == [(tokens, d, 0.0)]
    (dctx,) = [g for g in log.gemms if g["shape"] == (tokens, d, d) and g["b_kmajor"] and not g["a_kmajor"] and g["Cb"]]
    assert dctx["drop_p"] == 0.0 and not dctx["residual"] and not dctx["gate"] and not dctx["bias"] and dctx["splits"] == 1
    assert log.epilogues == []
    log.gemms.clear()
    log.grad_drops.clear()
