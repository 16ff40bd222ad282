"""GPU: the GEMM-path FFN the encoder runs below FUSED_FFN_MIN_TOKENS tokens per step (ltr_mi355x.encoder.ffn_gemm_fwd /
ffn_gemm_bwd, as _run_forward / _body_backward call them), against fp64.  The suite forces the fused FFN kernels on (tests/conftest.py); every test here picks its path
itself with LTR_ENC_FUSED_FFN.

  * kernels: the split-K activation GEMMs of that path (forward hid W2^T and input-gradient dz1 W1 layouts) slice by slice and
    summed, the split-K epilogue (bias + dropout + residual after the reduce) against fp64 and against gemm()'s own fused
    epilogue, the error returns, and the bf16 hidden tensor the path writes (bit-for-bit the fp32 result rounded to nearest even);
  * network: train-mode parity with the rounding-faithful fp64 oracle under exported dropout masks at every split-K factor the
    path takes at small steps, with counting wrappers proving which GEMMs ran (test_encoder_gpu.FfnCalls).

Bars: kernels on bf16-representable inputs, fp32 accumulation: 2e-5 of the tensor's max (test_encoder_gpu.py); the epilogue alone
(a handful of fp32 adds and one multiply per element): 1e-6; the network: the oracle gate of test_encoder_gpu.py."""
import copy

import pytest
import torch

from conftest import ledger_record
from test_encoder_gpu import FfnCalls, _oracle_gate, bits, err, rnd, unbits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BK = 64                 # k-step of gemm_bf16_kernel (csrc/ltr_encoder.hip)


@pytest.fixture(scope="module")
def enc():
    from ltr_mi355x import encoder
    return encoder


def _slices(K, ks):
    """k-range of every slice of gemm_bf16_kernel's split-K partition: ceil(ksteps / ks) whole k-steps each, the last one ragged."""
    ksteps = (K + BK - 1) // BK
    per = (ksteps + ks - 1) // ks
    return [(min(z * per * BK, K), min((z + 1) * per * BK, K)) for z in range(ks)]


# ------------------------------------------------------------------------------------------------- split-K activation GEMMs
@pytest.mark.parametrize("b_kmajor", [False, True], ids=["hid_W2T", "dz1_W1"])
@pytest.mark.parametrize("M,N,K,ks", [(384, 128, 1024, 2), (512, 128, 1536, 3), (4096, 128, 2048, 4),     # the heuristic's ks
                                      (1200, 136, 2048, 4),        # M and N tails, d_model 136
                                      (300, 24, 1000, 3),          # K % 64 != 0: the last slice ends inside a k-step
                                      (77, 24, 512, 5),            # 8 k-steps, 2 per slice: the fifth slice has none
                                      (9000, 128, 2048, 3)])       # LTR_ENC_FUSED_FFN=0 at 8 320 .. 10 880 tokens
def test_split_k_activation_gemm(enc, M, N, K, ks, b_kmajor):
    """C = A B^T (forward: hid [T][d_ff] x W2 [d][d_ff]) or A B (input gradient: dz1 [T][d_ff] x W1 [d_ff][d], B read k-major) into
    ks fp32 partials: every slice against fp64 over its own k-range, a slice without k-steps exactly zero, the fixed-order
    reduce against the fp64 product."""
    torch.manual_seed(M + N + K + ks + int(b_kmajor))
    A = rnd(M, K)
    Bm = rnd(K, N, scale=0.2) if b_kmajor else rnd(N, K, scale=0.2)
    Bkn = Bm if b_kmajor else Bm.t()                    # [K][N] view for the reference
    parts = torch.full((ks, M, N), float("nan"), device=DEV)
    enc.gemm(bits(A), bits(Bm), M, N, K, b_kmajor=b_kmajor, Cf=parts, splits=ks)
    sl = _slices(K, ks)
    empty = [z for z, (k0, k1) in enumerate(sl) if k0 == k1]
    if (M, N, K, ks) == (77, 24, 512, 5):
        assert empty == [4]
    for z, (k0, k1) in enumerate(sl):
        if k0 == k1:
            assert torch.equal(parts[z], torch.zeros(M, N, device=DEV)), z
        else:
            assert err(parts[z], A[:, k0:k1] @ Bkn[k0:k1]) < 2e-5, (z, k0, k1)
    got = enc.sum_partials(parts, ks, M * N).view(M, N)
    assert err(got, A @ Bkn) < 2e-5


# ------------------------------------------------------------------------------------------------- split-K epilogue
@pytest.mark.parametrize("with_bias,with_res", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("nsplit", [1, 2, 3, 4, 5])
def test_splitk_epilogue_vs_fp64(enc, nsplit, p, with_bias, with_res):
    """out = residual + keep (sum_s parts[s] + bias) / (1 - p) at M N / 4 = 680 000 quads, above the 2 048 x 256 threads of the
    grid: the grid-stride loop runs.  Without a residual the zeros are exactly the dropped elements of the exported mask."""
    M, N, seed, sid = 20000, 136, 0xFEEDFACE12345678, 19
    torch.manual_seed(nsplit * 100 + int(p * 10) + 2 * with_bias + with_res)
    parts = torch.randn(nsplit, M, N, device=DEV)
    bias = torch.randn(N, device=DEV) if with_bias else None
    res = torch.randn(M, N, device=DEV) * 2 if with_res else None
    out = torch.full((M, N), float("nan"), device=DEV)
    assert enc.splitk_epilogue(parts, nsplit, M, N, bias, p, seed, sid, res, out) is out
    assert bool(torch.isfinite(out).all())
    keep = enc.dropout_mask(seed, sid, M * N, p, DEV).view(M, N).double()
    v = parts.double().sum(0) + (bias.double() if with_bias else 0.0)
    want = v * keep / (1 - p) + (res.double() if with_res else 0.0)
    assert err(out, want) < 1e-6
    if not with_res:
        # zeros: the dropped elements, plus a kept one whose fp32 sum (the kernel's order: slice 0, 1, ..., then the bias) is exactly 0
        # -- over 2.7 M sums of normal draws that happens (about one in 10^7)
        v32 = parts[0].clone()
        for s in range(1, nsplit):
            v32 += parts[s]
        if with_bias:
            v32 += bias
        exact_zero = v32 == 0
        assert int(exact_zero.sum()) <= 4
        assert torch.equal(out == 0, (keep == 0) | exact_zero)
    if p == 0.0:
        assert bool((keep == 1).all())


def test_splitk_epilogue_matches_the_gemm_epilogue(enc):
    """The split-K path of the FFN output (ks partials + splitk_epilogue) against gemm()'s own epilogue (splits = 1) on the same
    inputs, seed and stream: the same dropped elements, bit for bit, and the same values up to the summation order."""
    M, N, K, ks, p, seed, sid = 4096, 128, 2048, 4, 0.1, 0x0123456789ABCDEF, 3
    torch.manual_seed(41)
    hid, w2 = rnd(M, K), rnd(N, K, scale=0.05)
    bias, res = torch.randn(N, device=DEV), torch.randn(M, N, device=DEV)
    keep = enc.dropout_mask(seed, sid, M * N, p, DEV).view(M, N)
    parts = torch.empty(ks, M, N, device=DEV)
    enc.gemm(bits(hid), bits(w2), M, N, K, Cf=parts, splits=ks)
    for r in (res, None):
        fused = torch.full((M, N), float("nan"), device=DEV)
        enc.gemm(bits(hid), bits(w2), M, N, K, Cf=fused, bias=bias, residual=r, drop_p=p, seed=seed, drop_stream=sid)
        split = torch.full((M, N), float("nan"), device=DEV)
        enc.splitk_epilogue(parts, ks, M, N, bias, p, seed, sid, r, split)
        dropped = keep == 0
        if r is None:
            assert torch.equal(fused == 0, dropped) and torch.equal(split == 0, dropped)
        else:
            assert torch.equal(fused[dropped], r[dropped]) and torch.equal(split[dropped], r[dropped])
        assert err(split, fused) < 1e-6
        want = (hid @ w2.t() + bias.double()) * keep.double() / (1 - p) + (0.0 if r is None else r.double())
        assert err(split, want) < 2e-5 and err(fused, want) < 2e-5


def test_splitk_epilogue_errors(enc):
    from ltr_mi355x._lib import LtrError
    M, N = 8, 16
    parts, out = torch.randn(2, M, N, device=DEV), torch.full((M, N), 7.0, device=DEV)
    enc.splitk_epilogue(parts, 2, 0, N, None, 0.1, 1, 0, None, out)            # M = 0: nothing to do, nothing written
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    with pytest.raises(LtrError):
        enc.splitk_epilogue(torch.randn(2, M, 6, device=DEV), 2, M, 6, None, 0.0, 1, 0, None, torch.empty(M, 6, device=DEV))  # N % 4
    with pytest.raises(LtrError):
        enc.splitk_epilogue(parts, 0, M, N, None, 0.0, 1, 0, None, out)         # nsplit = 0
    with pytest.raises(LtrError):
        enc.splitk_epilogue(parts, 2, M, N, None, 1.0, 1, 0, None, out)         # p = 1
    with pytest.raises(LtrError):
        enc.splitk_epilogue(None, 2, M, N, None, 0.0, 1, 0, None, out)          # parts = NULL
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ------------------------------------------------------------------------------------------------- hidden layer (bf16 out)
@pytest.mark.parametrize("T,dff,d,p", [(384, 1024, 128, 0.1), (1200, 2048, 136, 0.1), (77, 2048, 64, 0.0), (4096, 2048, 128, 0.5)])
def test_hidden_gemm_bf16_output_is_the_rounded_fp32_result(enc, T, dff, d, p):
    """hid = drop(relu(n2 W1^T + b1)) as the GEMM path writes it (bf16): requested together with the fp32 result in one launch,
    the bf16 tensor is the fp32 one rounded to nearest even, bit for bit (a truncating rounder stays inside 2^-8 of the max)."""
    torch.manual_seed(T + dff + d)
    seed, sid = 4242, 2
    n2, w1, b1 = rnd(T, d), rnd(dff, d, scale=0.15), torch.randn(dff, device=DEV) * 0.2
    Cf = torch.full((T, dff), float("nan"), device=DEV)
    Cb = torch.zeros(T, dff, dtype=torch.int16, device=DEV)
    enc.gemm(bits(n2), bits(w1), T, dff, d, Cf=Cf, Cb=Cb, bias=b1, relu=True, drop_p=p, seed=seed, drop_stream=sid)
    keep = enc.dropout_mask(seed, sid, T * dff, p, DEV).view(T, dff).double()
    want = torch.relu(n2 @ w1.t() + b1.double()) * keep / (1 - p)
    assert err(Cf, want) < 2e-5
    assert torch.equal(Cb.view(torch.bfloat16), Cf.to(torch.bfloat16))
    assert err(unbits(Cb), want) < 5e-3


# ------------------------------------------------------------------------------------------------- network, train mode
@pytest.mark.parametrize("d,dff,h,ks", [(128, 1024, 8, 2), (128, 1536, 8, 3), (128, 2048, 8, 4), (64, 2048, 4, 4), (136, 2048, 8, 4)])
def test_default_path_train_mode_matches_oracle_under_exported_masks(enc, monkeypatch, d, dff, h, ks):
    """A training step of a two-block make_model network at 384 tokens on the default (GEMM) FFN path, dropout 0.1 at every site,
    padded documents: the gradients against the rounding-faithful fp64 oracle fed the masks the kernels drew; the counting wrappers
    show the split-K GEMMs and epilogue ran with the ks named here."""
    import ltr_encoder_oracle as EO
    from architeture.multiLayer import make_model
    from losses.approxNDCG import approxNDCGLoss
    monkeypatch.delenv("LTR_ENC_FUSED_FFN", raising=False)
    F, B, S, N, p = 136, 6, 64, 2, 0.1
    T = B * S
    assert not enc.fused_ffn_enabled(d, dff, T) and enc._small_step_splits(T, d, dff) == ks
    torch.manual_seed(d + dff)
    fc = dict(sizes=[d], input_norm=False, activation=None, dropout=p)
    tr = dict(N=N, d_ff=dff, h=h, dropout=p, positional_encoding=None)
    net = make_model(copy.deepcopy(fc), copy.deepcopy(tr), dict(d_output=1, output_activation=None), F).to(DEV).train()
    x = torch.randn(B, S, F, device=DEV)
    y = torch.randint(0, 5, (B, S), device=DEV).float()
    mask = torch.zeros(B, S, dtype=torch.bool, device=DEV)
    mask[1, 50:] = True
    mask[4, 9:] = True
    y[mask] = -1
    net.ltr_seed = 91
    calls = FfnCalls(monkeypatch, enc)
    scores = net(x, mask, None)
    approxNDCGLoss(scores, y).backward()
    torch.cuda.synchronize()
    calls.assert_gemm_path(T, d, dff, N, ks, p)
    seed = (91 + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
    keep = {("fc", 0): enc.dropout_mask(seed, enc.stream_fc(0), T * d, p, DEV).view(T, d).cpu()}
    for l in range(N):
        keep[("attn", l)] = enc.attn_dropout_mask(seed, enc.stream_attn(l), B, S, h, p, DEV).cpu()
        keep[("attn_out", l)] = enc.dropout_mask(seed, enc.stream_attn_out(l), T * d, p, DEV).view(T, d).cpu()
        keep[("ffn_hidden", l)] = enc.dropout_mask(seed, enc.stream_ffn_hidden(l), T * dff, p, DEV).view(T, dff).cpu()
        keep[("ffn_out", l)] = enc.dropout_mask(seed, enc.stream_ffn_out(l), T * d, p, DEV).view(T, d).cpu()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    cfg = EO.config_of(dict(fc_model=fc, transformer=tr), F)
    got = {k: q.grad.cpu().double() for k, q in net.named_parameters()}
    gate = _oracle_gate(got, scores, sd, x, mask, cfg, y, keep=keep, what=f"default-FFN train d{d} dff{dff}")
    note = f"GEMM-path FFN, split-K ks={ks}; bf16 bars, tests/test_encoder_gpu.py"
    ledger_record("encoder train-mode [default FFN, split-K] worst param-grad vs rounding-faithful oracle under exported masks (max-norm)",
                  gate["max"], noise=gate["noise_max"], tol=max(2e-2, 4 * gate["noise_max"]), note=note + f"; min cosine {gate['min_cos']:.6f}")
    ledger_record("encoder train-mode [default FFN, split-K] worst param-grad vs rounding-faithful oracle under exported masks (L2)",
                  gate["l2"], noise=gate["noise_l2"], tol=max(1.5e-2, 2 * gate["noise_l2"]), note=note)
