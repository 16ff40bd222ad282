"""GPU: what each custom autograd Function's backward gets from its forward, when the caller does something between the two calls.

Every other GPU test runs `forward` and `backward` back to back.  Training code does not always: between them it may replay another
network's captured step, run a second forward, call backward twice with retain_graph=True, or change a parameter or input in place.
One table below has an entry per torch.autograd.Function of ltr_mi355x (one per variant that takes its own code path); every entry
calls `Fn.apply(...)` with an EXPLICIT seed.  Its baseline is the gradient of every differentiable input from forward + backward run
back to back at dropout epoch E.  Checked against that baseline, bit for bit (the kernels are free of float atomics, and repeats are
bitwise elsewhere in the suite):
  (a) epoch moved: seed_advance / seed_set / one replay of a GraphedTrainStep of a second network between forward and backward
      (entries that draw encoder dropout; include/ltr_encoder.h) -- the backward draws the forward's masks and leaves the epoch where
      it found it.  One oracle-gated network case on top: the gradient is the right one, not only a repeatable one;
  (b) interleaved calls: forward 1, forward 2 (other inputs, seed and epoch), backward 2, backward 1;
  (c) backward twice with retain_graph=True accumulates exactly 2 x the baseline;
  (d) an optimizer-style in-place change of one tensor argument between forward and backward: torch's "modified by an inplace
      operation" error (what the reference's nn modules raise) or the baseline gradient.  Anything else fails.
tests/test_autograd_state_cpu.py checks that the table names every Function of the package."""
import copy
import zlib

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
E0 = 4242                   # the epoch of every baseline
SEEDS = (0x1234567890ABCDEF, 0x0F1E2D3C4B5A6978, 0x5555AAAA3333CCCC)


@pytest.fixture(scope="module")
def enc():
    assert torch.cuda.is_available()
    import ltr_mi355x
    ltr_mi355x.lib()
    from ltr_mi355x import encoder
    yield encoder
    encoder.seed_set(0)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------- table
class Entry:
    """`make(gen)`: the tensor arguments {name: tensor} (differentiable ones are leaves with requires_grad), drawn from the CPU
    generator `gen`; `call(t, seed)`: Fn.apply(...) on them.  `enc_dropout`: the entry draws encoder dropout (scenario a)."""

    def __init__(self, fn, name, make, call, enc_dropout=False, env=None):
        self.fn, self.name, self.make, self.call, self.enc_dropout, self.env = fn, name, make, call, enc_dropout, env or {}

    def __repr__(self):
        return self.name


def _rand(gen, *shape, scale=1.0, lo=None, hi=None, grad=False, dtype=torch.float32):
    if lo is not None:
        v = lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)
    else:
        v = scale * torch.randn(shape, generator=gen, dtype=torch.float64)
    return v.to(dtype).to(DEV).requires_grad_(grad)


def _labels(gen, B, S, n=5, pad=True, dtype=torch.float32):
    y = torch.randint(0, n, (B, S), generator=gen).to(torch.float64)
    if pad:
        y[1, S - 5:] = -1.0
    return y.to(dtype).to(DEV)


def _fn(module, name):
    import importlib
    return getattr(importlib.import_module(f"ltr_mi355x.{module}"), name)


B, S = 4, 24


def _slates(gen, dtype=torch.float32, n_base=0):
    t = {"y_pred": _rand(gen, B, S, grad=True), "y_true": _labels(gen, B, S, dtype=dtype)}
    if n_base:
        t["y_base"] = _rand(gen, B, S, n_base)
    return t


def _functional_entries():
    F = lambda n: _fn("functional", n)                                                          # noqa: E731
    return [
        Entry("ApproxNDCG", "ApproxNDCG", _slates, lambda t, s: F("ApproxNDCG").apply(t["y_pred"], t["y_true"], 1e-10, -1.0, 1.0)),
        Entry("ListNet", "ListNet", _slates, lambda t, s: F("ListNet").apply(t["y_true"], t["y_pred"], False)),
        Entry("LambdaLoss", "LambdaLoss", _slates,
              lambda t, s: F("LambdaLoss").apply(t["y_pred"], t["y_true"], 1e-10, -1, "ndcgLoss2PP_scheme", None, 1.0, 10.0, "sum", "binary")),
        Entry("LambdaPairs", "LambdaPairs-fp32-labels", _slates,
              lambda t, s: F("LambdaPairs").apply(t["y_pred"], t["y_true"], 1e-10, -1, "ndcgLoss2PP_scheme", None, 1.0, 10.0, "binary")),
        Entry("LambdaPairs", "LambdaPairs-fp64-labels", lambda g: _slates(g, dtype=torch.float64),
              lambda t, s: F("LambdaPairs").apply(t["y_pred"], t["y_true"], 1e-10, -1, "ndcgLoss2PP_scheme", None, 1.0, 10.0, "binary")),
        Entry("Ordinal", "Ordinal", lambda g: {"y_pred": _rand(g, B, S, 4, lo=0.05, hi=0.95, grad=True), "y_true": _labels(g, B, S)},
              lambda t, s: F("Ordinal").apply(t["y_pred"], t["y_true"], 4, -1)),
    ]


def _risk_entries():
    R = lambda n: _fn("risk", n)                                                                # noqa: E731
    Q = 12
    return [
        Entry("RiskEval", "RiskEval-geo", lambda g: {"mat": _rand(g, Q, 4, lo=0.1, hi=0.9, grad=True)},
              lambda t, s: R("RiskEval").apply(t["mat"], 2.0, 0, 1)),
        Entry("TRisk", "TRisk", lambda g: {"model": _rand(g, Q, lo=0.1, hi=0.9, grad=True), "baseline": _rand(g, Q, lo=0.1, hi=0.9, grad=True)},
              lambda t, s: R("TRisk").apply(t["model"], t["baseline"], 2.0)),
        Entry("LambdaColsum", "LambdaColsum", _slates,
              lambda t, s: R("LambdaColsum").apply(t["y_pred"], t["y_true"], 1e-10, -1, "ndcgLoss2PP_scheme", None, 1.0, 10.0, "binary")),
        Entry("LambdaColsumSys", "LambdaColsumSys", lambda g: _slates(g, n_base=3),
              lambda t, s: R("LambdaColsumSys").apply(t["y_pred"], t["y_true"], t["y_base"], 1e-10, -1, "ndcgLoss2PP_scheme", None, 1.0,
                                                      10.0, "binary")),
        Entry("LambdaRiskLoss", "LambdaRiskLoss", lambda g: _slates(g, n_base=3),
              lambda t, s: R("LambdaRiskLoss").apply(t["y_pred"], t["y_true"], t["y_base"], "ndcgLoss2PP_scheme", 2, True, False, 1, 2.0, 1,
                                                     False, 1.0)),
        Entry("RiskMatrix", "RiskMatrix", lambda g: {"ref": _labels(g, B, S, pad=False), "x0": _rand(g, B, S, grad=True),
                                                     "rest": _rand(g, B, S, 3)},
              lambda t, s: R("RiskMatrix").apply(t["ref"], t["x0"], t["rest"], 0, 2, True)),
        Entry("RiskTail", "RiskTail", lambda g: {"mat": _rand(g, Q, 4, lo=0.1, hi=0.9, grad=True)},
              lambda t, s: R("RiskTail").apply(t["mat"], 2.0, 1, 1, True, 1.0, False)),
        Entry("TRiskTail", "TRiskTail", lambda g: {"mat": _rand(g, Q, 2, lo=0.1, hi=0.9, grad=True)},
              lambda t, s: R("TRiskTail").apply(t["mat"], 2.0, True, 1.0)),
    ]


_DOUBLE136 = [(136, 136), (136,), (136, 136), (136,), (1, 136), (1,)]
_TRIPLE136 = [(64, 136), (64,), (32, 64), (32,), (1, 32), (1,)]
_TWO64H = [(64, 136), (64,), (1, 64), (1,)]
N_DOCS = B * S


def _mlp_make(shapes, keep=False):
    def make(g):
        t = {"x": _rand(g, B, S, 136)}
        for i, sh in enumerate(shapes):
            a = (6.0 / (sh[0] + sh[1])) ** 0.5 if len(sh) == 2 else 0.1
            t[f"p{i}"] = _rand(g, *sh, lo=-a, hi=a, grad=True)
        if keep:
            t["keep1"] = (torch.rand((N_DOCS, 136), generator=g) >= 0.5).to(torch.uint8).to(DEV)
            t["keep2"] = (torch.rand((N_DOCS, 136), generator=g) >= 0.5).to(torch.uint8).to(DEV)
        return t
    return make


def _mlp_call(net_name, p=None):
    def call(t, seed):
        from ltr_mi355x import scorer as SC
        net = getattr(SC, net_name)
        params = [t[k] for k in sorted(t) if k.startswith("p")]
        code = 0 if p is None else SC.drop_code(True, p)
        return SC._MLPScores.apply(t["x"], net, code, seed & (2 ** 64 - 1), t.get("keep1"), t.get("keep2"), *params)
    return call


def _scorer_entries():
    return [
        Entry("_MLPScores", "MLP-double-p0.5", _mlp_make(_DOUBLE136), _mlp_call("NET_DOUBLE", 0.5)),
        Entry("_MLPScores", "MLP-double-p0.3-saved-acts", _mlp_make(_DOUBLE136), _mlp_call("NET_DOUBLE", 0.3)),
        Entry("_MLPScores", "MLP-double-explicit-keep", _mlp_make(_DOUBLE136, keep=True), _mlp_call("NET_DOUBLE", 0.5)),
        Entry("_MLPScores", "MLP-triple-folded", _mlp_make(_TRIPLE136), _mlp_call("NET_TRIPLE"), env={"LTR_TRIPLE_FOLD": "1"}),
        Entry("_MLPScores", "MLP-136-64-1", _mlp_make(_TWO64H), _mlp_call("NET_TWO_LAYER_64H")),
    ]


# the encoder network of the EncoderScores / Features entries: 24 features -> FC 64 -> two blocks (4 heads, d_ff 128), slates of 20
EB, ES, EF, ED, EDFF, EH = 3, 20, 24, 64, 128, 4


def _spec(input_norm=False, fc_p=0.2, enc_p=0.1):
    from ltr_mi355x.encoder import EncoderSpec
    return EncoderSpec(EF, [ED], input_norm, fc_p, 2, EH, EDFF, enc_p, True)


def _enc_params(g, input_norm):
    """{name: leaf} in EncoderScores' parameter order (the names sort in that order)."""
    shapes = []
    if input_norm:
        shapes += [("ln", (EF,)), ("ln", (EF,))]
    shapes += [("W", (ED, EF)), ("b", (ED,))]
    for _ in range(2):
        shapes += [("ln", (ED,)), ("ln", (ED,))] + [("W", (ED, ED)), ("b", (ED,))] * 4 + [("ln", (ED,)), ("ln", (ED,)),
                                                                                           ("W", (EDFF, ED)), ("b", (EDFF,)),
                                                                                           ("W", (ED, EDFF)), ("b", (ED,))]
    shapes += [("ln", (ED,)), ("ln", (ED,)), ("W", (1, ED)), ("b", (1,))]
    out = {}
    for i, (kind, sh) in enumerate(shapes):
        if kind == "W":
            a = (6.0 / (sh[0] + sh[1])) ** 0.5
            v = _rand(g, *sh, lo=-a, hi=a, grad=True)
        elif kind == "ln" and (i % 2 == 0):
            v = (1.0 + 0.1 * torch.randn(sh, generator=g, dtype=torch.float64)).float().to(DEV).requires_grad_(True)
        else:
            v = _rand(g, *sh, scale=0.1, grad=True)
        out[f"p{i:03d}"] = v
    return out


def _enc_make(input_norm=False, x_grad=False, drop_tail=0):
    """drop_tail: leave out the last parameters (Features takes no output layer, and without its final norm not that either)."""
    def make(g):
        mask = torch.zeros(EB, ES, dtype=torch.bool)
        mask[1, 15:] = True
        mask[2, 18:] = True
        t = {"x": _rand(g, EB, ES, EF, grad=x_grad), "mask": mask.to(DEV)}
        prm = _enc_params(g, input_norm)
        for k in sorted(prm)[len(prm) - drop_tail:]:
            del prm[k]
        t.update(prm)
        return t
    return make


def _params_of(t):
    return [t[k] for k in sorted(t) if k.startswith("p")]


def _enc_call(training=True, input_norm=False):
    def call(t, seed):
        from ltr_mi355x.encoder import EncoderScores
        return EncoderScores.apply(_spec(input_norm), t["x"], t["mask"], seed, training, *_params_of(t))
    return call


def _features_call(final_norm):
    def call(t, seed):
        from ltr_mi355x.blocks import Features
        return Features.apply(_spec(), final_norm, t["x"], t["mask"], seed, True, *_params_of(t))
    return call


def _encoder_entries():
    return [
        Entry("EncoderScores", "Encoder-train-fused-ffn", _enc_make(), _enc_call(), enc_dropout=True, env={"LTR_ENC_FUSED_FFN": "1"}),
        Entry("EncoderScores", "Encoder-train-gemm-ffn", _enc_make(), _enc_call(), enc_dropout=True, env={"LTR_ENC_FUSED_FFN": "0"}),
        Entry("EncoderScores", "Encoder-eval", _enc_make(), _enc_call(training=False)),
        Entry("EncoderScores", "Encoder-train-input-norm", _enc_make(input_norm=True), _enc_call(input_norm=True), enc_dropout=True),
    ]


def _mask_u8(g):
    m = torch.zeros(EB, ES, dtype=torch.uint8)
    m[1, 15:] = 1
    m[2, 18:] = 1
    return m.to(DEV)


def _mha_make(same):
    def make(g):
        t = {"query": _rand(g, EB, ES, ED, grad=True)}
        if not same:
            t["key"], t["value"] = _rand(g, EB, ES, ED, grad=True), _rand(g, EB, ES, ED, grad=True)
        t["mask_u8"] = _mask_u8(g)
        a = (6.0 / (2 * ED)) ** 0.5
        for i in range(4):
            t[f"p{2 * i}"] = _rand(g, ED, ED, lo=-a, hi=a, grad=True)
            t[f"p{2 * i + 1}"] = _rand(g, ED, scale=0.1, grad=True)
        return t
    return make


def _mha_call(same):
    def call(t, seed):
        from ltr_mi355x.blocks import MultiHeadFn
        q = t["query"]
        k, v = (q, q) if same else (t["key"], t["value"])
        return MultiHeadFn.apply(EH, 0.1, seed, same, q, k, v, t["mask_u8"], *_params_of(t))
    return call


def _blocks_entries():
    from_blocks = lambda n: _fn("blocks", n)                                                     # noqa: E731
    ln_make = lambda g: {"x": _rand(g, EB, ES, ED, grad=True), "a": (1.0 + 0.1 * _rand(g, ED)).detach().requires_grad_(True),   # noqa: E731
                         "b": _rand(g, ED, scale=0.1, grad=True)}
    lin_make = lambda n: (lambda g: {"x": _rand(g, EB, ES, ED, grad=True), "W": _rand(g, n, ED, lo=-0.3, hi=0.3, grad=True),   # noqa: E731
                                     "b": _rand(g, n, scale=0.1, grad=True)})

    def attn_make(g):
        t = {k: _rand(g, EB, EH, ES, ED // EH, grad=True) for k in ("query", "key", "value")}
        t["mask_u8"] = _mask_u8(g)
        return t

    def ffn_make(g):
        a = (6.0 / (ED + EDFF)) ** 0.5
        return {"x": _rand(g, EB, ES, ED, grad=True), "W1": _rand(g, EDFF, ED, lo=-a, hi=a, grad=True), "b1": _rand(g, EDFF, scale=0.1, grad=True),
                "W2": _rand(g, ED, EDFF, lo=-a, hi=a, grad=True), "b2": _rand(g, ED, scale=0.1, grad=True)}

    return [
        Entry("Features", "Features-final-norm", _enc_make(x_grad=True, drop_tail=2), _features_call(True), enc_dropout=True),
        Entry("Features", "Features-no-final-norm", _enc_make(x_grad=True, drop_tail=4), _features_call(False), enc_dropout=True),
        Entry("LayerNormFn", "LayerNorm-standard", ln_make, lambda t, s: from_blocks("LayerNormFn").apply(t["x"], t["a"], t["b"], 1e-5, 1)),
        Entry("LayerNormFn", "LayerNorm-transformer", ln_make, lambda t, s: from_blocks("LayerNormFn").apply(t["x"], t["a"], t["b"], 1e-6, 0)),
        Entry("LinearFn", "Linear-padded-N", lin_make(5), lambda t, s: from_blocks("LinearFn").apply(t["x"], t["W"], t["b"])),
        Entry("ScoreLinearFn", "ScoreLinear", lin_make(1), lambda t, s: from_blocks("ScoreLinearFn").apply(t["x"], t["W"], t["b"])),
        Entry("MultiHeadFn", "MultiHead-self", _mha_make(True), _mha_call(True), enc_dropout=True),
        Entry("MultiHeadFn", "MultiHead-cross", _mha_make(False), _mha_call(False), enc_dropout=True),
        Entry("AttentionCoreFn", "AttentionCore", attn_make,
              lambda t, s: from_blocks("AttentionCoreFn").apply(t["query"], t["key"], t["value"], t["mask_u8"], 0.1, s), enc_dropout=True),
        Entry("FeedForwardFn", "FeedForward", ffn_make,
              lambda t, s: from_blocks("FeedForwardFn").apply(0.2, s, t["x"], t["W1"], t["b1"], t["W2"], t["b2"]), enc_dropout=True),
    ]


ENTRIES = _functional_entries() + _risk_entries() + _scorer_entries() + _encoder_entries() + _blocks_entries()
FUNCTIONS = sorted({e.fn for e in ENTRIES})
ENC_DROPOUT = [e for e in ENTRIES if e.enc_dropout]


# ------------------------------------------------------------------------------------------------------------- runner
def _env(monkeypatch, entry):
    for k, v in entry.env.items():
        monkeypatch.setenv(k, v)


def _fresh(entry, k):
    """The tensor arguments of call k (k = 0, 1, 2: different values)."""
    return entry.make(torch.Generator().manual_seed(zlib.crc32(entry.name.encode()) + 7919 * k))


def _forward(entry, t, k):
    out = entry.call(t, SEEDS[k])
    return out[0] if isinstance(out, tuple) else out


def _cotangent(out, k):
    g = torch.Generator().manual_seed(101 + k)
    return torch.randn(out.shape, generator=g, dtype=torch.float64).to(out.dtype).to(out.device)


def _leaves(t):
    seen, out = set(), {}
    for n, v in t.items():
        if v.requires_grad and id(v) not in seen:
            seen.add(id(v))
            out[n] = v
    return out


def _grads(t):
    return {n: None if v.grad is None else v.grad.clone() for n, v in _leaves(t).items()}


def _baseline(entry, k, epoch, enc):
    t = _fresh(entry, k)
    enc.seed_set(epoch)
    out = _forward(entry, t, k)
    out.backward(_cotangent(out, k))
    g = _grads(t)
    assert all(v is not None for v in g.values()), (entry.name, "baseline without a gradient", [n for n, v in g.items() if v is None])
    return g


def _diff(got, want, factor=1):
    """Tensors that are not bit-identical to factor x want: [(name, max |delta|)]."""
    bad = []
    for n, w in want.items():
        w = w * factor
        g = got.get(n)
        if g is None or g.dtype != w.dtype or g.shape != w.shape:
            bad.append((n, "missing or of another dtype / shape"))
        elif not torch.equal(g, w):
            bad.append((n, float((g.double() - w.double()).abs().max())))
    return bad


# ------------------------------------------------------------------------------------------------------------- (a)
@pytest.fixture(scope="module")
def other_step(enc):
    """One captured training step of a second, independent network with encoder dropout: a replay bumps the epoch first."""
    from architeture.multiLayer import make_model
    from losses.approxNDCG import approxNDCGLoss
    from ltr_mi355x.graphs import GraphedTrainStep
    torch.manual_seed(11)
    fc = dict(sizes=[64], input_norm=False, activation=None, dropout=0.1)
    tr = dict(N=1, d_ff=128, h=4, dropout=0.1, positional_encoding=None)
    net = make_model(fc, tr, dict(d_output=1, output_activation=None), 16).to(DEV).train()
    x = torch.randn(2, 16, 16, device=DEV)
    y = torch.randint(0, 5, (2, 16), device=DEV).float()
    mask = torch.zeros(2, 16, dtype=torch.bool, device=DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3, capturable=True)
    step = GraphedTrainStep(net, opt, lambda n, x_, m_, y_: approxNDCGLoss(n(x_, m_, None), y_), (x, mask, y), warmup=2)
    return lambda: step(x, mask, y)


@pytest.mark.parametrize("move", ["advance", "set", "graph_replay"])
@pytest.mark.parametrize("entry", ENC_DROPOUT, ids=repr)
def test_epoch_moved_between_forward_and_backward(enc, other_step, monkeypatch, entry, move):
    _env(monkeypatch, entry)
    want = _baseline(entry, 0, E0, enc)
    t = _fresh(entry, 0)
    enc.seed_set(E0)
    out = _forward(entry, t, 0)
    if move == "advance":
        enc.seed_advance(1)
    elif move == "set":
        enc.seed_set(E0 + 12345)
    else:
        other_step()
    before = enc.seed_get()
    assert before != E0
    out.backward(_cotangent(out, 0))
    after = enc.seed_get()
    bad = _diff(_grads(t), want)
    assert not bad, (entry.name, move, "gradient differs from the back-to-back baseline", bad)
    assert after == before, (entry.name, move, "the backward left the epoch changed", before, after)


def test_network_epoch_moved_matches_oracle_under_forward_masks(enc):
    """A two-block network in training mode, forward at epoch E_f, the epoch moved before the backward: the gradients against the
    rounding-faithful fp64 oracle fed the masks of seed + E_f (the forward's)."""
    import ltr_encoder_oracle as EO
    from architeture.multiLayer import make_model
    from losses.approxNDCG import approxNDCGLoss
    from test_encoder_gpu import _oracle_gate
    torch.manual_seed(5)
    F, Bn, Sn = 24, 3, 40
    fc = dict(sizes=[48, 32], input_norm=False, activation=None, dropout=0.2)
    tr = dict(N=2, d_ff=64, h=4, dropout=0.1, positional_encoding=None)
    net = make_model(copy.deepcopy(fc), copy.deepcopy(tr), dict(d_output=1, output_activation=None), F).to(DEV).train()
    x = torch.randn(Bn, Sn, F, device=DEV)
    y = torch.randint(0, 5, (Bn, Sn), device=DEV).float()
    mask = torch.zeros(Bn, Sn, dtype=torch.bool, device=DEV)
    mask[1, 30:] = True
    y[mask] = -1
    net.ltr_seed = 77
    E_f = 31337
    enc.seed_set(E_f)
    scores = net(x, mask, None)
    enc.seed_advance(5)
    approxNDCGLoss(scores, y).backward()
    assert enc.seed_get() == E_f + 5
    enc.seed_set(0)
    seed = (77 + 0x9E3779B97F4A7C15 + E_f) & (2 ** 64 - 1)
    T, d, dff, h = Bn * Sn, 32, 64, 4
    keep = {("fc", 0): enc.dropout_mask(seed, enc.stream_fc(0), T * 48, 0.2, DEV).view(T, 48).cpu(),
            ("fc", 1): enc.dropout_mask(seed, enc.stream_fc(1), T * 32, 0.2, DEV).view(T, 32).cpu()}
    for l in range(2):
        keep[("attn", l)] = enc.attn_dropout_mask(seed, enc.stream_attn(l), Bn, Sn, h, 0.1, DEV).cpu()
        keep[("attn_out", l)] = enc.dropout_mask(seed, enc.stream_attn_out(l), T * d, 0.1, DEV).view(T, d).cpu()
        keep[("ffn_hidden", l)] = enc.dropout_mask(seed, enc.stream_ffn_hidden(l), T * dff, 0.1, DEV).view(T, dff).cpu()
        keep[("ffn_out", l)] = enc.dropout_mask(seed, enc.stream_ffn_out(l), T * d, 0.1, DEV).view(T, d).cpu()
    sd = {k: v.detach().cpu() for k, v in net.state_dict().items()}
    cfg = EO.config_of(dict(fc_model=fc, transformer=tr), F)
    got = {k: p.grad.cpu().double() for k, p in net.named_parameters()}
    _oracle_gate(got, scores, sd, x, mask, cfg, y, keep=keep, what="train-mode dropout, epoch moved")


# ------------------------------------------------------------------------------------------------------------- (b), (c)
@pytest.mark.parametrize("entry", ENTRIES, ids=repr)
def test_interleaved_forwards_and_backwards(enc, monkeypatch, entry):
    _env(monkeypatch, entry)
    E1, E2 = E0 + 1, E0 + 1000
    want1, want2 = _baseline(entry, 1, E1, enc), _baseline(entry, 2, E2, enc)
    t1, t2 = _fresh(entry, 1), _fresh(entry, 2)
    enc.seed_set(E1)
    o1 = _forward(entry, t1, 1)
    enc.seed_set(E2)
    o2 = _forward(entry, t2, 2)
    o2.backward(_cotangent(o2, 2))
    o1.backward(_cotangent(o1, 1))
    bad1, bad2 = _diff(_grads(t1), want1), _diff(_grads(t2), want2)
    assert not bad1 and not bad2, (entry.name, "call 1", bad1, "call 2", bad2)


@pytest.mark.parametrize("entry", ENTRIES, ids=repr)
def test_backward_twice_accumulates_twice_the_gradient(enc, monkeypatch, entry):
    _env(monkeypatch, entry)
    want = _baseline(entry, 0, E0, enc)
    t = _fresh(entry, 0)
    enc.seed_set(E0)
    out = _forward(entry, t, 0)
    g = _cotangent(out, 0)
    out.backward(g, retain_graph=True)
    out.backward(g, retain_graph=True)
    bad = _diff(_grads(t), want, factor=2)
    assert not bad, (entry.name, "two backwards are not 2 x the baseline", bad)


# ------------------------------------------------------------------------------------------------------------- (d)
def _nudge(v):
    """An optimizer-style in-place change: floats += 1/16; integer / bool tensors (masks) flip their last element."""
    with torch.no_grad():
        if v.dtype.is_floating_point:
            v.add_(0.0625)
        elif v.dtype == torch.bool:
            v.view(-1)[-1:].logical_not_()
        else:
            v.view(-1)[-1:].bitwise_xor_(1)


@pytest.mark.parametrize("entry", ENTRIES, ids=repr)
def test_inplace_change_between_forward_and_backward(enc, monkeypatch, entry):
    _env(monkeypatch, entry)
    want = _baseline(entry, 0, E0, enc)
    names = list(_fresh(entry, 0))
    bad, raised = [], []
    for name in names:
        t = _fresh(entry, 0)
        enc.seed_set(E0)
        out = _forward(entry, t, 0)
        _nudge(t[name])
        try:
            out.backward(_cotangent(out, 0))
        except RuntimeError as e:
            if "modified by an inplace operation" in str(e):
                raised.append(name)
            else:
                bad.append((name, "raised", str(e)[:200]))
            continue
        d = _diff(_grads(t), want)
        if d:
            bad.append((name, "neither raised nor returned the baseline", d))
    assert not bad, (entry.name, bad)
    assert enc.seed_get() == E0, (entry.name, "a failed backward left the epoch changed")
