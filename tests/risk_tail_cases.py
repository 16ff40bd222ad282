"""Case builders shared by tests/test_risk_tails_cpu.py and tests/test_risk_tails_gpu.py (a plain module, no fixtures).

The two tails of the risk losses (`risk_tail_kernel`, `trisk_tail_kernel` in csrc/ltr_risk.hip) run as ONE workgroup of 1024 threads
that sweeps the rows of the [queries x systems] matrix: thread t owns rows t, t + 1024, ...; a wave is 64 rows.  TAIL_Q sits on both
sides of every wave and sweep edge.  The matrix kernel runs 256 threads per query over slates of up to 2048 documents: MATRIX_S sits on
both sides of every multiple of 256 that changes the number of strided iterations.  Everything here is CPU code against the fp64
oracle; the preconditions below are checked by test_risk_tails_cpu.py before any GPU time is spent.

Variants of the matrix (fp32 numbers before the kernel or the oracle sees them):
  plain           uniform in [0.1, 0.9].
  max_ties2       plain, with the maximum TIE planted twice: (row 0, column 0) and (row Q - 1, last column).
  max_ties_third  the maximum planted about Q / 3 times (at least twice), rows spread evenly over 0 .. Q - 1 and always including rows
                  0, Q / 2 and Q - 1, columns cycling through 0, the middle one and the last one (row 0 -> column 0, row Q / 2 -> the
                  middle column, row Q - 1 -> the last column): the tied entries belong to different threads, waves and sweeps.
  model_worse     every entry times a rung of WORSE_LADDER (the first that lands in the window), column 0 times WORSE_DROP on two rows out of three (the model fails on most queries):
                  zRisk / Q of the model at alpha = 5 lies in (-5.5, -2.5), the regime where an fp32 normal cdf 0.5 (1 + erf) cancels
                  (tests/golden/make_golden_r2.py).  Below -5.5 the fp64 oracle's own 1 + erf starts to cancel, so the window is two-sided.
  equal_rows      every row the same, so every residual d_q is 0 up to rounding: the VALUE is compared absolutely and the gradient is
                  not compared (the sign of a rounding residue decides between the weights 1 and 1 + alpha).  The row's maximum sits in
                  the middle column (n >= 3) or the last one (n = 2), so that the flip does not zero column 0.  With n = 2 the flip
                  zeroes the whole last column: strategies 2 / 3 are then 0 / 0 exactly like the one-system flip (expect_nan below).  Q = 1
                  runs this variant only (one row is "every row the same").  Not a tRisk variant: equal deltas have std 0.

Non-numeric outcomes, asserted as NaN on both sides and nothing else: tRisk at Q = 1 (std of one sample), one system with the flip
(the only column becomes e = 0 where the maximum sits), and a column that the flip turns into all zeros (equal_rows, n = 2, strategies
2 / 3: the same 0 / 0 in the last column).
"""
import functools
from collections import namedtuple

import numpy as np
import torch

import ltr_risk_oracle as RO

TAIL_Q = (2, 3, 63, 64, 65, 1023, 1024, 1025, 2047, 2049, 4097)
TAIL_N = (2, 3, 9)
WIDE = (1025, 65)                       # (Q, n): the widest row a cached step can produce, at one Q
ONE_SYSTEM = (37, 1)                    # flipped: 0 / 0 on both sides; unflipped: e_q = x_q, every residual 0
VARIANTS = ("plain", "max_ties2", "max_ties_third", "model_worse", "equal_rows")
T_VARIANTS = ("plain", "max_ties2", "max_ties_third", "model_worse")
ALPHAS = (0.0, 1.0, 5.0)
FACTORS = (1.0, -1.0)
TIE = 0.95                              # above every uniform entry
WORSE_LADDER, WORSE_DROP, WORSE_WINDOW = (7.0, 14.0, 28.0), 0.02, (-5.5, -2.5)
GAP = 1e-3                              # strategies 2 / 3: |R1 - R0| >= GAP max(|R0|, |R1|) in the fp64 oracle
BIAS_LADDER = (1.0, 0.8, 0.6, 0.4)      # factor on the last column (before ties are planted): independent uniform columns have
                                        # nearly equal risks at large Q, so a seed may miss GAP; the first rung that meets it is taken

Opt = namedtuple("Opt", "geo strategy zquirk flip alpha factor")
TOpt = namedtuple("TOpt", "flip alpha factor")


def options():
    """Both kinds x strategies 1, 2, 3 (the z kind's strategy 2 with and without the precedence quirk) x flip x alpha x factor."""
    out = []
    for geo in (True, False):
        for strategy, zq in ((1, False), (2, False), (3, False)) + (() if geo else ((2, True),)):
            for flip in (False, True):
                for alpha in ALPHAS:
                    for f in FACTORS:
                        out.append(Opt(geo, strategy, zq, flip, alpha, f))
    return out


def t_options():
    return [TOpt(flip, alpha, f) for flip in (False, True) for alpha in ALPHAS for f in FACTORS]


def opt_id(o):
    if isinstance(o, TOpt):
        return f"t-{'flip' if o.flip else 'noflip'}-a{o.alpha:g}-f{o.factor:g}"
    return f"{'geo' if o.geo else 'z'}-s{o.strategy}{'q' if o.zquirk else ''}-{'flip' if o.flip else 'noflip'}-a{o.alpha:g}-f{o.factor:g}"


def tail_shapes():
    """(Q, n, variant) of the geo / z tail: every Q x every n x every variant, Q = 1 (equal_rows), the wide row at one Q, one system."""
    out = [(1, n, "equal_rows") for n in TAIL_N]
    out += [(Q, n, v) for Q in TAIL_Q for n in TAIL_N for v in VARIANTS]
    out += [WIDE + (v,) for v in VARIANTS]
    out.append(ONE_SYSTEM + ("plain",))
    return out


def absolute(variant, Q, n):
    """Every residual is 0 up to rounding (equal rows, one query, one system): value compared absolutely, gradient not compared."""
    return variant == "equal_rows" or Q == 1 or n == 1


def t_shapes():
    return [(Q, v) for Q in TAIL_Q for v in T_VARIANTS]


def q_regime(Q):
    return "Q <= 1024" if Q <= 1024 else "Q > 1024"


# ------------------------------------------------------------------------------------------------- matrices
def tie_positions(variant, Q, n):
    """[(row, column)] of the planted maxima; [] for a variant without them."""
    if variant == "max_ties2":
        return [(0, 0), (Q - 1, n - 1)]
    if variant != "max_ties_third":
        return []
    c = max(2, int(round(Q / 3.0)))
    rows = sorted({int(round(i * (Q - 1) / (c - 1))) for i in range(c)} | {0, Q // 2, Q - 1})
    mid = n // 2
    out = []
    for i, r in enumerate(rows):
        col = (0, mid, n - 1)[i % 3]
        if r == Q // 2:
            col = mid
        if r == Q - 1:
            col = n - 1
        if r == 0:
            col = 0
        out.append((r, col))
    return out


def _plain(Q, n, bias=1.0):
    gen = torch.Generator().manual_seed(500 + 100 * Q + n)
    m = torch.rand(Q, n, generator=gen) * 0.8 + 0.1
    m[:, n - 1] = m[:, n - 1] * bias
    return m


def _variant(variant, Q, n, bias, scale):
    m = _plain(Q, n, bias)
    if variant in ("max_ties2", "max_ties_third"):
        for r, c in tie_positions(variant, Q, n):
            m[r, c] = TIE
    elif variant == "model_worse":
        m = m * scale
        drop = torch.arange(Q) % 3 != 0
        m[drop, 0] = m[drop, 0] * WORSE_DROP
    elif variant == "equal_rows":
        row = m[0].clone()
        j, want = int(row.argmax()), (n // 2 if n >= 3 else n - 1)
        row[j], row[want] = row[want].clone(), row[j].clone()
        m = row[None, :].repeat(Q, 1)
    elif variant != "plain":
        raise KeyError(variant)
    return m.contiguous()


def worse_v(m):
    """zRisk / Q of the model (column 0) at alpha = 5, fp64 oracle."""
    return float(RO.z_risk(m.double(), 5.0, 0)) / m.shape[0]


@functools.lru_cache(maxsize=None)
def recipe(variant, Q, n):
    """(last-column bias, model_worse scale) of a case: the first rung of each ladder that meets the case's preconditions; raises if
    none does.  No case is ever dropped for a precondition: the input changes instead."""
    scales = WORSE_LADDER if variant == "model_worse" else (1.0,)
    if absolute(variant, Q, n):
        return 1.0, scales[0]
    for scale in scales:
        if variant == "model_worse" and not WORSE_WINDOW[0] < worse_v(_variant(variant, Q, n, 1.0, scale)) < WORSE_WINDOW[1]:
            continue
        for bias in BIAS_LADDER:
            m = _variant(variant, Q, n, bias, scale)
            if gaps_ok(m) and (variant != "model_worse" or WORSE_WINDOW[0] < worse_v(m) < WORSE_WINDOW[1]):
                return bias, scale
    raise AssertionError(f"no rung of the ladders meets the preconditions of {variant} Q{Q} n{n}")


@functools.lru_cache(maxsize=None)
def _matrix(variant, Q, n):
    return _variant(variant, Q, n, *recipe(variant, Q, n))


def matrix(variant, Q, n):
    """The fp32 [Q, n] matrix of a case (a fresh copy)."""
    return _matrix(variant, Q, n).clone()


def risks64(m, geo, flip, alpha):
    """(R0, R1) of the fp64 oracle as Python floats."""
    _, r0, r1 = RO.risk_tail_parts(m.double(), alpha, geo, 2, flip, 1.0)
    return float(r0), float(r1)


def gaps_ok(m):
    """Strategies 2 / 3: |R1 - R0| >= GAP max(|R0|, |R1|) in the fp64 oracle, both kinds, flip off and on, every alpha."""
    for geo in (True, False):
        for flip in (False, True):
            for alpha in ALPHAS:
                r0, r1 = risks64(m, geo, flip, alpha)
                if not abs(r1 - r0) >= GAP * max(abs(r0), abs(r1)):
                    return False
    return True


def expect_nan(variant, n, opt):
    """The 0 / 0 cases of the geo / z tail (module docstring)."""
    if not opt.flip:
        return False
    return n == 1 or (variant == "equal_rows" and n == 2 and opt.strategy > 1)


def ulp32(x):
    """One fp32 unit in the last place of |x|."""
    return float(np.spacing(np.float32(abs(x))))


def rounding_allowance(opt, r0, r1, value):
    """(for the value, for the gradient) added to the bar of strategies 2 / 3.  The kernel rounds R0 and R1 to fp32 before combining
    them, where the reference does: each moves by at most half an ulp, their combination by at most u = ulp32(max(|R0|, |R1|)).
      strategy 2: value f (R1 - R0) [quirk: f R1 - R0] is off by u, relative u / |value|  (= u / |R1 - R0| without the quirk);
                  the gradient does not depend on R0 / R1.
      strategy 3: value f (R1 - R0)^2 is off by 2 u |R1 - R0|, relative 2 u / |R1 - R0|; the gradient's coefficients +-2 f (R1 - R0)
                  are off by 2 u, relative u / |R1 - R0|.
    R0, R1 and the value come from the fp64 oracle."""
    if opt.strategy == 1:
        return 0.0, 0.0
    u = ulp32(max(abs(r0), abs(r1)))
    if opt.strategy == 2:
        return u / abs(value), 0.0
    return 2.0 * u / abs(r1 - r0), u / abs(r1 - r0)


# ------------------------------------------------------------------------------------------------- blocks
BLOCK_Q = (3, 64, 1024, 1025, 2047, 2049, 4097)
CANARY = -12345.0
Layout = namedtuple("Layout", "name n_blocks block_rows counts")


def layouts(Q):
    """Block layouts of a dense matrix of Q rows: (n_blocks, block_rows) in {(1, Q), (2, ceil(Q / 2)), (3, ..), (8, ..), (1024, 2)}."""
    h = -(-Q // 2)
    out = [Layout("one_full", 1, Q, (Q,)), Layout("two_ragged_last", 2, h, (h, Q - h)),
           Layout("three_empty_first", 3, h, (0, h, Q - h))]
    r, left, c = -(-Q // 5), Q, []
    for k in range(8):                                       # an empty middle block, two empty trailing blocks
        take = 0 if k in (2, 6, 7) else min(r, left)
        c.append(take)
        left -= take
    assert left == 0
    out.append(Layout("eight_empty_middle_and_tail", 8, r, tuple(c)))
    if Q % 8 == 0:
        out.append(Layout("eight_full", 8, Q // 8, (Q // 8,) * 8))
    if Q <= 2048:                                            # the 1024-block limit: 2, 1, 0, 2 rows, topped up from the end
        c, left = [], Q
        for k in range(1024):
            take = min((2, 1, 0, 2)[k % 4], left)
            c.append(take)
            left -= take
        for k in range(1023, -1, -1):
            add = min(2 - c[k], left)
            c[k] += add
            left -= add
        assert left == 0
        out.append(Layout("limit_1024_blocks", 1024, 2, tuple(c)))
    if Q > 1024:
        out.append(Layout("boundary_at_row_1024", 2, max(1024, Q - 1024), (1024, Q - 1024)))
        mid = min(48, Q - 1000)
        out.append(Layout("block_straddles_row_1024", 3, max(1000, Q - 1000 - mid), (1000, mid, Q - 1000 - mid)))
    return out


def pack(mat, layout, pad=float("nan")):
    """[n_blocks, 1 + block_rows * n]: block k = its row count as a float, its rows, then `pad`."""
    Q, n = mat.shape
    assert sum(layout.counts) == Q and len(layout.counts) == layout.n_blocks and max(layout.counts) <= layout.block_rows
    out = torch.full((layout.n_blocks, 1 + layout.block_rows * n), pad, dtype=mat.dtype)
    at = 0
    for k, c in enumerate(layout.counts):
        out[k, 0] = float(c)
        out[k, 1:1 + c * n] = mat[at:at + c].reshape(-1)
        at += c
    return out


def unpack(blocks, n):
    """The valid rows of packed blocks, in block order (counts read from the headers)."""
    rows = [blocks[k, 1:1 + int(blocks[k, 0]) * n].reshape(-1, n) for k in range(blocks.shape[0])]
    return torch.cat(rows, 0)


def unpack_like(packed, blocks, n):
    """The rows of `packed` (a tensor in the blocks' layout, e.g. dmat) that are valid in `blocks`."""
    rows = [packed[k, 1:1 + int(blocks[k, 0]) * n].reshape(-1, n) for k in range(blocks.shape[0])]
    return torch.cat(rows, 0)


def padding_mask(layout, n):
    """True where a packed float is a header or padding (what a launch must leave alone in dmat)."""
    m = torch.ones((layout.n_blocks, 1 + layout.block_rows * n), dtype=torch.bool)
    for k, c in enumerate(layout.counts):
        m[k, 1:1 + c * n] = False
    return m


# ------------------------------------------------------------------------------------------------- matrix rows
MATRIX_S = (1, 2, 3, 63, 65, 255, 256, 257, 511, 513, 1023, 1025, 2047, 2048)
MATRIX_B = 3
MATRIX_NREST = (0, 1, 3)


def matrix_inputs(S, mode, n_rest):
    """(ref, x0, rest) fp32.  Modes 0 / 2: labels 0..4, scores randn, rest [B, S, n_rest].  Mode 1: vectors taken as they are, of the
    size and sign of lambdaMask column sums of soft-maxed scores (negative, order 1), rest [n_rest, B, S]."""
    gen = torch.Generator().manual_seed(800 + 10 * S + mode)
    B = MATRIX_B
    if mode == 1:
        ref = -(torch.rand(B, S, generator=gen) + 0.1)
        x0 = -(torch.rand(B, S, generator=gen) + 0.1)
        rest = -(torch.rand(n_rest, B, S, generator=gen) + 0.1) if n_rest else None
    else:
        ref = torch.randint(0, 5, (B, S), generator=gen).float()
        x0 = torch.randn(B, S, generator=gen)
        rest = torch.randn(B, S, n_rest, generator=gen) if n_rest else None
    return ref, x0, rest


def matrix_oracle(ref, x0, rest, mode, lt, ideal, dtype):
    """(mat [B, 1 + n_rest + ideal], jac [B, S] = d mat[b, 0] / d x0[b, :]) of the oracle in `dtype`, unflipped."""
    x = x0.detach().clone().to(dtype).requires_grad_(True)
    t = ref.to(dtype)
    r = None if rest is None else rest.to(dtype)
    if mode == 1:
        systems = [x] + ([] if r is None else [r[k] for k in range(r.shape[0])]) + ([t] if ideal else [])
        if lt == 1:
            cols = [((s - t) ** 2).sum(dim=1) for s in systems]
        elif lt == 2:
            cols = [RO._cos(t, s) for s in systems]
        else:
            cols = [(s.sum(dim=1) - t.sum(dim=1)) ** 2 for s in systems]
        mat = torch.stack(cols, dim=1)
    else:
        sm = lambda v: torch.softmax(v, dim=1)              # (RO._softmaxes squeezes: a slate or a baseline of one would vanish)
        pt, pp, pb = sm(t), sm(x), None if r is None else sm(r)
        if mode == 2 and lt == 2:                             # the tRisk pair: cosine of the PRODUCTS (riskLosses.py:256-258)
            systems = [pp] + ([] if pb is None else [pb[:, :, j] for j in range(pb.shape[2])]) + ([pt] if ideal else [])
            mat = torch.stack([RO._t_cols(pt * pt, pt * p, pt * p, 2)[0] for p in systems], dim=1)
        else:
            mat = RO.listnet_matrix(pt, pp, pb, lt, 2 if ideal else 1, flip=False)
    jac, = torch.autograd.grad(mat[:, 0].sum(), x)
    return mat.detach(), jac

