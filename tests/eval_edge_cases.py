"""Case builders shared by tests/test_eval_edges_cpu.py and tests/test_eval_edges_gpu.py (a plain module, no fixtures, no GPU).

The small kernels around the training hot path, each at the edges of its launch geometry:

  NDCG@k (csrc/ltr_metrics.hip)      one workgroup per query, block = clamp(next_pow2(S), 64, 1024), 8 S bytes of dynamic LDS: more than
                                     64 KiB above S = 8192 (the hipFuncSetAttribute opt-in), S <= 16384.  NDCG_SHAPES sits on both sides
                                     of 64, 1024, 2048 and 8192 and on the limit; ROW_KINDS are the rows a ranker really produces.
  ordinal loss (csrc/ltr_losses.hip) 256 documents per workgroup, then reduce_pairs_kernel (1024 threads, strided by 1024 over the block
                                     partials): a second stride needs more than 1024 x 256 documents.  ORDINAL_CASES.
  ltr_reduce_sum_f32                 one workgroup of 1024 threads = 16 waves.  REDUCE_N, REDUCE_SCALES, reduce_bound.
  gather (csrc/ltr_data.hip)         narrow / scalar: grid-stride above 256 * 32 workgroups of 256 lanes; wide (rows of >= 512 float4):
                                     pieces of 1024 float4, grid-stride above 256 * 64 workgroups.  GATHER_CASES.

Every input comes from a seeded host generator.  Metric inputs are fp32-representable (the device ranks in fp32, the oracle in fp64:
both must see one order); test_eval_edges_cpu.py asserts that, and that no builder drops a case.
"""
import functools
import math
from collections import namedtuple

import numpy as np
import torch

# ------------------------------------------------------------------------------------------------- NDCG@k, dense
NDCG_SHAPES = ((3, 63), (3, 64), (3, 65), (2, 1023), (2, 1024), (2, 1025), (2, 2048), (2, 2049), (2, 8192), (2, 8193), (1, 16384))
NDCG_S_LIMIT = 16384
FULL_PRODUCT_UP_TO = 1025                # the full option cross product up to this S, five option sets beyond (ndcg_options)
ROW_KINDS = ("normal5", "quant4", "all_equal", "signed_zero", "no_relevant", "relevant_last", "fractional", "negative")
QUANT_LEVELS = (-1.5, -0.25, 0.25, 2.0)

NdcgOpt = namedtuple("NdcgOpt", "k gains no_relevant reverse_ties want")


def _labels5(rng, S):
    return rng.integers(0, 5, size=S).astype(np.float64)


def ndcg_row(kind, S, seed):
    """(labels [S] float64, scores [S] float32) of one row kind.
      normal5        random normal scores, five-level integer labels (LETOR): label ties in the ideal DCG, score ties by accident only
      quant4         scores quantised to 4 values: tie runs of about S / 4 documents, what reverse_ties reorders
      all_equal      one score for every document (a collapsed ranker): the order IS the tie rule
      signed_zero    random scores with +0.0 and -0.0 planted alternately on every fourth document: they compare equal
      no_relevant    every label 0: ideal DCG 0, the result is the no_relevant value
      relevant_last  one relevant document, at the last index, tied with a quarter of the slate (quantised scores)
      fractional     labels on a 1 / 64 grid in [0, 4) (linear gains take any float; 2 ** y too)
      negative       labels in {-4 .. 0}: the ideal DCG is negative or 0, and utils/metrics.py only tests `== 0` before dividing"""
    rng = np.random.default_rng(seed)
    y = _labels5(rng, S)
    s = rng.standard_normal(S).astype(np.float32)
    if kind == "normal5":
        pass
    elif kind == "quant4":
        s = np.asarray(QUANT_LEVELS, dtype=np.float32)[rng.integers(0, 4, size=S)]
    elif kind == "all_equal":
        s = np.full(S, 0.375, dtype=np.float32)
    elif kind == "signed_zero":
        at = np.arange(0, S, 4)
        s[at] = np.where(np.arange(at.size) % 2 == 0, np.float32(0.0), np.float32(-0.0))
        s[S - 1] = np.float32(-0.0) if s[0] == 0 and not np.signbit(s[0]) else np.float32(0.0)
    elif kind == "no_relevant":
        y = np.zeros(S, dtype=np.float64)
    elif kind == "relevant_last":
        s = np.asarray(QUANT_LEVELS, dtype=np.float32)[rng.integers(0, 4, size=S)]
        y = np.zeros(S, dtype=np.float64)
        y[S - 1] = 3.0
    elif kind == "fractional":
        y = np.floor(rng.random(S) * 256.0) / 64.0
    elif kind == "negative":
        y = -y
    else:
        raise KeyError(kind)
    return y, s


def ndcg_batches(Q, S):
    """[(name, kinds)]: the row kinds dealt Q at a time, so that every kind appears at every shape and kinds mix within a batch."""
    out = []
    for a in range(0, len(ROW_KINDS), Q):
        kinds = tuple(ROW_KINDS[(a + i) % len(ROW_KINDS)] for i in range(Q))
        out.append(("+".join(kinds), kinds))
    return out


@functools.lru_cache(maxsize=None)
def _ndcg_batch(Q, S, kinds):
    rows = [ndcg_row(kind, S, 1000 * S + 10 * ROW_KINDS.index(kind) + i) for i, kind in enumerate(kinds)]
    y, s = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    y.setflags(write=False)
    s.setflags(write=False)
    return y, s


def ndcg_batch(Q, S, kinds):
    """(labels [Q, S] float64, scores [Q, S] float32), read-only, built once."""
    assert len(kinds) == Q
    return _ndcg_batch(Q, S, tuple(kinds))


def ndcg_ks(S):
    return (1, S - 1, S, S + 7, None) if S > 1 else (1, S + 7, None)


def ndcg_options(S):
    """Up to S = 1025: k x gains x no_relevant x reverse_ties x want.  Beyond: five sets, every k once, both gains, both no_relevant
    values, both tie rules and both `want` values at least twice."""
    if S <= FULL_PRODUCT_UP_TO:
        return [NdcgOpt(k, g, nr, rev, w) for k in ndcg_ks(S) for g in ("linear", "exponential") for nr in (True, False)
                for rev in (False, True) for w in ("ndcg", "dcg")]
    return [NdcgOpt(1, "linear", True, False, "ndcg"), NdcgOpt(S - 1, "exponential", False, True, "dcg"),
            NdcgOpt(S, "linear", False, True, "ndcg"), NdcgOpt(S + 7, "exponential", True, False, "dcg"),
            NdcgOpt(None, "exponential", True, True, "ndcg")]


def ndcg_opt_id(o):
    return f"k{o.k}-{o.gains[:3]}-nr{int(o.no_relevant)}-{'rev' if o.reverse_ties else 'fwd'}-{o.want}"


def ndcg_dense_cases():
    """[(Q, S, batch name, kinds)] -- the parametrisation of the dense NDCG tests."""
    return [(Q, S, name, kinds) for Q, S in NDCG_SHAPES for name, kinds in ndcg_batches(Q, S)]


def ndcg_reference(MO, y, s, o):
    """The oracle's per-query value of one option set (k = None: every document)."""
    k = y.shape[1] if o.k is None else o.k
    if o.want == "dcg":
        return MO.dcg_at_k(y, s, k, o.gains, stable=not o.reverse_ties)
    return MO.ndcg_per_query(y, s, k=k, no_relevant=o.no_relevant, gains=o.gains, stable=not o.reverse_ties)


# ------------------------------------------------------------------------------------------------- NDCG@k, ragged
RAGGED_LENGTHS = (1, 2, 63, 64, 65, 128, 129, 1024, 1025, 2048)        # tier edges of ltr_mi355x.ragged.TIER_HI, two queries each
RAGGED_KS = (1, 10, None)
RAGGED_EQUAL_S = (64, 65, 1024)                                         # ragged == dense bit for bit
RAGGED_EQUAL_Q = 4


@functools.lru_cache(maxsize=None)
def ragged_batch():
    """(labels [n_docs] float64, scores [n_docs] float32, bounds [Q + 1] int64): each length twice, normal5 then quant4."""
    ys, ss, lengths = [], [], []
    for L in RAGGED_LENGTHS:
        for kind in ("normal5", "quant4"):
            y, s = ndcg_row(kind, L, 77000 + 10 * L + ROW_KINDS.index(kind))
            ys.append(y)
            ss.append(s)
            lengths.append(L)
    bounds = np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)
    out = np.concatenate(ys), np.concatenate(ss), bounds
    for a in out:
        a.setflags(write=False)
    return out


def ragged_equal_batch(S):
    """(labels, scores) [RAGGED_EQUAL_Q, S] of an equal-length batch: normal5, quant4, all_equal, signed_zero."""
    return ndcg_batch(RAGGED_EQUAL_Q, S, ROW_KINDS[:RAGGED_EQUAL_Q])


# ------------------------------------------------------------------------------------------------- ordinal
ORD_BLOCK = 256                          # kOrdBlock
ORD_STRIDE = 1024                        # reduce_pairs_kernel's threads: block partials beyond this take a second stride
SMALLEST_NORMAL = float(np.finfo(np.float32).tiny)                     # 2 ** -126
SUBNORMAL = float(np.float32(1e-41))
NEAR_ONE = 1.0 - 2.0 ** -24
CLAMP_P = (0.0, 1.0, SMALLEST_NORMAL, SUBNORMAL, NEAR_ONE)
CLAMP_DOCS = (0, 63, 64, 255, 256)       # flat document index of each CLAMP_P value: three waves, two workgroups

OrdCase = namedtuple("OrdCase", "name B S n pad labels clamp y64 go")


def _ord(name, B, S, n, pad=-1, labels="mixed", clamp=False, y64=False, go=1.0):
    return OrdCase(name, B, S, n, pad, labels, clamp, y64, go)


ORDINAL_CASES = (
    _ord("docs1-n1", 1, 1, 1, labels="valid"),
    _ord("docs255-n5", 5, 51, 5),
    _ord("docs256-n2", 4, 64, 2),
    _ord("docs257-n64", 1, 257, 64),                                   # n = 64: the ABI maximum
    _ord("docs257-n5-fp64-labels", 257, 1, 5, y64=True),
    _ord("docs256-n5-upstream3", 2, 128, 5, go=3.0),
    _ord("docs262144-n1-one-stride", 512, 512, 1),                     # 1024 workgroups: reduce_pairs_kernel's loop runs once
    _ord("docs262145-n2-second-stride", 5, 52429, 2),                  # 1025 workgroups: thread 0 takes a second partial
    _ord("docs278528-n1-second-stride-6pct", 544, 512, 1),             # 1088 workgroups: 64 partials, 5.9 % of the documents, in the
                                                                       # second stride -- leaving it out moves loss or gradient past 1e-5
    _ord("docs257-n5-pad0", 1, 257, 5, pad=0),                         # masks the 0 TARGETS, keeps a padded document's -1 targets
    _ord("docs257-n5-pad1", 1, 257, 5, pad=1),                         # masks the 1 TARGETS
    _ord("docs262145-n2-pad0", 5, 52429, 2, pad=0),
    _ord("docs257-n5-clamp", 1, 257, 5, clamp=True),
    _ord("docs257-n5-clamp-pad0", 1, 257, 5, pad=0, clamp=True),
    _ord("docs257-n5-clamp-pad1", 1, 257, 5, pad=1, clamp=True),
    _ord("docs257-n5-all-padded", 1, 257, 5, labels="all_padded"),     # 0 / 0
    _ord("docs256-n2-pad0-all-zero-labels", 4, 64, 2, pad=0, labels="all_zero"),       # every target 0 = pad: 0 / 0 again
)


def ordinal_label_values(n):
    """-1 (padding), 0 .. n, n + 2 (above every ordinal) and 2.5 (`y >= k` on a fraction)."""
    return [-1.0] + [float(v) for v in range(n + 1)] + [float(n + 2), 2.5]


@functools.lru_cache(maxsize=None)
def _ordinal_inputs(name):
    c = next(x for x in ORDINAL_CASES if x.name == name)
    gen = torch.Generator().manual_seed(9000 + ORDINAL_CASES.index(c))
    p = torch.rand(c.B, c.S, c.n, generator=gen) * 0.98 + 0.01
    vals = torch.tensor(ordinal_label_values(c.n))
    if c.labels == "mixed":
        y = vals[torch.randint(0, vals.numel(), (c.B, c.S), generator=gen)]
        flat = y.view(-1)
        flat[: min(vals.numel(), flat.numel())] = vals[: flat.numel()]   # every label value at least once (where there is room)
    elif c.labels == "valid":
        y = torch.ones(c.B, c.S)
    elif c.labels == "all_padded":
        y = torch.full((c.B, c.S), -1.0)
    elif c.labels == "all_zero":
        y = torch.zeros(c.B, c.S)
    else:
        raise KeyError(c.labels)
    if c.B * c.S > ORD_STRIDE * ORD_BLOCK:
        y.view(-1)[-1] = 1.0             # label 1 has an unmasked target under every pad: the second stride always holds valid documents
    clamp = torch.zeros(c.B * c.S, dtype=torch.bool)
    if c.clamp:
        assert c.n >= 2 and c.B * c.S > max(CLAMP_DOCS)
        pf, yf = p.view(-1, c.n), y.view(-1)
        for doc, v in zip(CLAMP_DOCS, CLAMP_P):
            pf[doc] = torch.tensor(v, dtype=torch.float32)               # every slot: label 1 gives targets (1, 0, 0, ..): both
            yf[doc] = 1.0
            clamp[doc] = True
    return p.contiguous(), y.contiguous(), clamp.view(c.B, c.S)


def ordinal_inputs(c):
    """(p [B, S, n] fp32, y [B, S] fp32 or fp64, clamp [B, S] bool: the documents that carry a CLAMP_P value).  Fresh copies."""
    p, y, clamp = _ordinal_inputs(c.name)
    return p.clone(), (y.double() if c.y64 else y.clone()), clamp.clone()


def ordinal_second_stride(c):
    """True where reduce_pairs_kernel needs a second stride: more than ORD_STRIDE workgroups of ORD_BLOCK documents."""
    return c.B * c.S > ORD_STRIDE * ORD_BLOCK


def ordinal_sums(O, p, y, n, pad, docs=None):
    """(sum of the unmasked BCE terms, number of valid documents) over the first `docs` documents (None: all) in fp64: what
    ltr_ordinal_fwd_bwd leaves in sums[0] / sums[1].  From the oracle: loss x count, and the count itself."""
    pf, yf = p.double().reshape(1, -1, n)[:, :docs], y.reshape(1, -1)[:, :docs]
    t = O.with_ordinals(yf, n)
    count = int(((t != pad).sum(2) > 0).sum())
    loss, _ = O.ordinal_closed_form(pf, yf, n, pad)
    return float(loss) * count, count


def ordinal_expect_nan(c):
    return c.labels in ("all_padded", "all_zero")


# ------------------------------------------------------------------------------------------------- reduce_sum
REDUCE_N = (0, 1, 63, 64, 65, 1023, 1024, 1025, 100003)     # 63 / 64 / 65: one wave slot, 15 (14) empty; 1023: the last lane idle
REDUCE_SCALES = (1.0, 1.0 / 7.0)


def reduce_input(n):
    """[max(n, 1)] fp32 (n = 0 still needs a pointer), mixed sign, |x| log-uniform in [1e-3, 1e3]."""
    rng = np.random.default_rng(4000 + n)
    m = max(n, 1)
    return (np.where(rng.random(m) < 0.5, -1.0, 1.0) * 10.0 ** rng.uniform(-3.0, 3.0, size=m)).astype(np.float32)


def reduce_reference(x, n, scale):
    """fsum of the first n fp32 values times the fp32 scale the kernel receives, in fp64."""
    return math.fsum(float(v) for v in x[:n]) * float(np.float32(scale))


def reduce_bound(x, n, scale):
    """|err| <= (ceil(n / 1024) + 22 + 1) 2^-24 sum|x| |scale|, from reduce_sum_kernel (csrc/ltr_losses.hip):
         for (i = threadIdx.x; i < n; i += 1024) a += in[i];      ceil(n / 1024) roundings on the longest chain
         a = wave_allsum(a);                                      6 shuffle levels (64 lanes)
         for (i = 0; i < 16; ++i) x += red[i];                    16 wave slots
         out[0] = x * scale;                                      1
    Every rounding is relative 2^-24 of a partial sum, and every partial sum is at most sum|x|."""
    terms = -(-n // 1024) + 22 + 1
    return terms * 2.0 ** -24 * float(np.abs(x[:n].astype(np.float64)).sum()) * abs(float(np.float32(scale)))


# ------------------------------------------------------------------------------------------------- gather
GatherCase = namedtuple("GatherCase", "name rows row_floats misaligned kernel")
GATHER_THREADS, NARROW_CAP, WIDE_CAP, WIDE_PIECE_F4, WIDE_FROM_F4 = 256, 256 * 32, 256 * 64, 1024, 512
GATHER_MAX_BYTES = 150_000_000
GATHER_CASES = (
    GatherCase("narrow-70000x128-second-stride", 70000, 128, False, "narrow"),        # 2.24 M float4 against 2 097 152 lanes
    GatherCase("scalar-300000x7-second-stride", 300000, 7, False, "scalar"),          # 2.1 M floats, rows of no whole float4
    GatherCase("scalar-misaligned-70000x128-second-stride", 70000, 128, True, "scalar"),
    GatherCase("wide-17000x2048-above-the-workgroup-cap", 17000, 2048, False, "wide"),  # 17 000 workgroups against 16 384
    GatherCase("narrow-300x2044-below-the-wide-edge", 300, 2044, False, "narrow"),    # 511 float4
    GatherCase("wide-300x2048-at-the-wide-edge", 300, 2048, False, "wide"),           # 512 float4: half a piece
    GatherCase("wide-300x4092-piece-minus-one", 300, 4092, False, "wide"),            # 1023 float4
    GatherCase("wide-300x4096-one-piece", 300, 4096, False, "wide"),                  # 1024 float4 exactly
    GatherCase("wide-300x4100-piece-plus-one", 300, 4100, False, "wide"),             # 1025 float4: a second piece of one float4
    GatherCase("wide-300x8192-two-pieces", 300, 8192, False, "wide"),
)


def gather_kernel_of(c):
    """The kernel ltr_gather_rows_f32 picks (csrc/ltr_data.hip): scalar unless rows are whole float4s at 16-byte-aligned pointers,
    wide from 512 float4 a row."""
    if c.misaligned or c.row_floats % 4:
        return "scalar"
    return "wide" if c.row_floats // 4 >= WIDE_FROM_F4 else "narrow"


def gather_strides(c):
    """How many grid-stride iterations the busiest workgroup runs."""
    k = gather_kernel_of(c)
    if k == "wide":
        pieces = -(-(c.row_floats // 4) // WIDE_PIECE_F4)
        return -(-(c.rows * pieces) // WIDE_CAP)
    total = c.rows * (c.row_floats // 4 if k == "narrow" else c.row_floats)
    return -(-(-(-total // GATHER_THREADS)) // NARROW_CAP)


def gather_source(c):
    """fp32 [rows, row_floats] from a seeded host generator; `misaligned`: a view one float into a larger buffer."""
    gen = torch.Generator().manual_seed(6000 + c.rows + c.row_floats + int(c.misaligned))
    n = c.rows * c.row_floats
    if c.misaligned:
        return torch.randn(n + 1, generator=gen)[1:].view(c.rows, c.row_floats)
    return torch.randn(n, generator=gen).view(c.rows, c.row_floats)


def gather_indices(c):
    """{name: (idx int64, bad bool)}: a permutation, a third of it, and the permutation with every 5th index negative (idx - rows,
    the same row) and every 7th out of range (rows, -rows - 1 and rows + 5 in turn: a zero row) -- spread over the whole launch, so
    the second grid-stride iteration meets them too."""
    gen = torch.Generator().manual_seed(7000 + c.rows + c.row_floats)
    perm = torch.randperm(c.rows, generator=gen)
    mixed = perm.clone()
    neg = torch.arange(0, c.rows, 5)
    mixed[neg] = perm[neg] - c.rows
    bad_at = torch.arange(3, c.rows, 7)
    mixed[bad_at] = torch.tensor([c.rows, -c.rows - 1, c.rows + 5])[torch.arange(bad_at.numel()) % 3]
    bad = torch.zeros(c.rows, dtype=torch.bool)
    bad[bad_at] = True
    none = torch.zeros(c.rows, dtype=torch.bool)
    return {"perm": (perm, none), "sub": (perm[: c.rows // 3].clone(), none[: c.rows // 3]), "mixed": (mixed, bad)}


def gather_expected(src, idx, bad):
    """src[idx] with torch's negative indexing, a zero row where the index is out of range."""
    safe = torch.where(bad, torch.zeros_like(idx), idx)
    out = src[safe]
    out[bad] = 0.0
    return out
