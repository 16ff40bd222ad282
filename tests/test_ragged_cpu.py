"""CPU: the host side of the ragged path (ltr_mi355x.ragged) -- RaggedSlates' offsets / tiers / batches / permutations against a
brute-force recomputation, argument rejection of the four ltr_*_ragged_* launchers before any device is touched, CPU tensors
refused, and the equivalence that makes the GPU tests' reference sound: the per-query oracle loop equals the fp64 oracle on the
-1-padded rectangle for approxNDCG and lambdaLoss."""
import numpy as np
import pytest
import torch

import lambda_tier_cases as LT
import ltr_oracle as O
import ragged_cases as RC


@pytest.fixture(scope="module")
def handle():
    from ltr_mi355x.build import build
    build(force=False, verbose=False)
    import ltr_mi355x
    return ltr_mi355x.lib()


def _lengths():
    rng = np.random.default_rng(5)
    extra = [int(v) for v in rng.integers(1, 2049, size=60)]
    mixed = list(LT.TIER_S) + extra + list(LT.TIER_S)
    return [int(v) for v in rng.permutation(np.asarray(mixed))]


def _brute_tiers(sizes):
    """{tier upper end: sorted query ids}: a length belongs to the first tier end that is >= it."""
    from ltr_mi355x.ragged import TIER_HI
    out = {}
    for q, s in enumerate(sizes):
        hi = next(h for h in TIER_HI if s <= h)
        out.setdefault(hi, []).append(q)
    return out


def _next_pow2(v):
    p = 1
    while p < v:
        p <<= 1
    return p


def _check_structure(sl, sizes):
    from ltr_mi355x.ragged import TIER_HI
    assert sl.n_queries == len(sizes) and sl.n_docs == sum(sizes) and sl.max_len == (max(sizes) if sizes else 0)
    assert sl.offsets_host.tolist() == [sum(sizes[:q]) for q in range(len(sizes) + 1)]
    brute = _brute_tiers(sizes)
    got = {}
    for s_max, a, n in sl.tiers():
        ids = sl.order_host[a:a + n].tolist()
        assert ids == sorted(ids) and n > 0
        lens = [sizes[q] for q in ids]
        assert s_max == max(lens)
        # the geometry rule: one power of two per launch; 256 never shares a launch with 129 .. 255 (lambdaLoss changes kernel there)
        assert {_next_pow2(v) for v in lens} == {_next_pow2(s_max)}
        assert not (256 in lens and min(lens) < 256)
        hi = next(h for h in TIER_HI if s_max <= h)
        got[hi] = ids
    assert got == brute
    assert sorted(sl.order_host.tolist()) == list(range(len(sizes)))


def test_slates_offsets_and_tiers_vs_brute_force():
    from ltr_mi355x.ragged import RaggedSlates
    sizes = _lengths()
    assert set(LT.TIER_S) <= set(sizes)
    sl = RaggedSlates(RC.bounds_of(sizes))
    _check_structure(sl, sizes)
    for q0, q1 in [(0, len(sizes)), (0, 1), (7, 8), (3, 40), (50, len(sizes)), (20, 20)]:
        b = sl.batch(q0, q1)
        _check_structure(b, sizes[q0:q1])
        assert sl.doc_range(q0, q1) == (sum(sizes[:q0]), sum(sizes[:q1]))
    with pytest.raises(ValueError):
        sl.batch(5, 3)
    with pytest.raises(ValueError):
        sl.batch(0, len(sizes) + 1)


def test_from_qid_matches_query_bounds():
    from ltr_mi355x.data import query_bounds
    from ltr_mi355x.ragged import RaggedSlates
    qid = np.repeat(np.array([7, 3, 3, 9, 1]), [4, 1, 2, 300, 17])      # equal neighbouring ids merge, as in the reference's reader
    sl = RaggedSlates.from_qid(qid)
    assert sl.offsets_host.tolist() == query_bounds(qid).tolist() == [0, 4, 7, 307, 324]
    assert sl.sizes.tolist() == [4, 3, 300, 17]


def test_permuted_round_trips():
    from ltr_mi355x.ragged import RaggedSlates
    sizes = _lengths()[:40]
    sl = RaggedSlates(RC.bounds_of(sizes))
    rng = np.random.default_rng(3)
    perm = rng.permutation(len(sizes))
    new, idx = sl.permuted(perm)
    _check_structure(new, [sizes[p] for p in perm])
    doc_q = np.repeat(np.arange(len(sizes)), sizes)                      # query of every old row
    moved = doc_q[idx.numpy()]
    assert moved.tolist() == np.repeat(perm, [sizes[p] for p in perm]).tolist()
    assert sorted(idx.tolist()) == list(range(sl.n_docs))
    inv = np.argsort(perm)
    back, idx2 = new.permuted(inv)
    assert back.offsets_host.tolist() == sl.offsets_host.tolist()
    assert idx[idx2].tolist() == list(range(sl.n_docs))
    with pytest.raises(ValueError):
        sl.permuted(np.zeros(len(sizes), dtype=np.int64))


@pytest.mark.parametrize("bounds", [[0, 3, 3, 5], [0, 2049], [0, 5, 4, 9], [1, 4], [0.0, 2.0], [[0, 1]]])
def test_bad_bounds_raise(bounds):
    from ltr_mi355x.ragged import RaggedSlates
    with pytest.raises(ValueError):
        RaggedSlates(np.asarray(bounds))


def test_slates_refuse_the_cpu_as_a_device():
    from ltr_mi355x import LtrDeviceError
    from ltr_mi355x.ragged import RaggedSlates
    with pytest.raises(LtrDeviceError):
        RaggedSlates([0, 3, 5]).to("cpu")


def test_ragged_argument_rejection_without_gpu(handle):
    """NULL pointers and bad shapes come back as LTR_ERR_* before a device is touched; 1 stands for a non-NULL pointer that the
    launchers must not get as far as using."""
    h = handle
    ok = 1 << 12          # a non-NULL address; every call below is rejected before anything reads it
    NULL, SHAPE, PARAM = -1, -2, -3
    for s_max, want in ((0, SHAPE), (2049, SHAPE), (-5, SHAPE)):
        assert h.ltr_approxndcg_ragged_fwd_bwd(ok, ok, ok, None, 3, s_max, 1.0, 1e-10, -1.0, 1.0, ok, None, None) == want
        assert h.ltr_listnet_ragged_fwd_bwd(ok, ok, ok, None, 3, s_max, 0, 1.0, ok, None, None) == want
        assert h.ltr_lambda_ragged_fwd_bwd(ok, ok, ok, None, 3, s_max, 4, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1.0, ok, ok, None, None) == want
        assert h.ltr_ndcg_at_k_ragged(ok, ok, ok, None, 3, s_max, 5, 0, 1, 0, ok, None, None) == want
    assert h.ltr_approxndcg_ragged_fwd_bwd(ok, ok, ok, None, -1, 8, 1.0, 1e-10, -1.0, 1.0, ok, None, None) == SHAPE
    assert h.ltr_listnet_ragged_fwd_bwd(ok, ok, ok, None, -1, 8, 0, 1.0, ok, None, None) == SHAPE
    assert h.ltr_lambda_ragged_fwd_bwd(ok, ok, ok, None, -1, 8, 4, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1.0, ok, ok, None, None) == SHAPE
    assert h.ltr_ndcg_at_k_ragged(ok, ok, ok, None, -1, 8, 5, 0, 1, 0, ok, None, None) == SHAPE
    # NULL scores / labels / offsets / outputs
    assert h.ltr_approxndcg_ragged_fwd_bwd(None, ok, ok, None, 3, 8, 1.0, 1e-10, -1.0, 1.0, ok, None, None) == NULL
    assert h.ltr_approxndcg_ragged_fwd_bwd(ok, ok, None, None, 3, 8, 1.0, 1e-10, -1.0, 1.0, ok, None, None) == NULL
    assert h.ltr_approxndcg_ragged_fwd_bwd(ok, ok, ok, None, 3, 8, 1.0, 1e-10, -1.0, 1.0, None, None, None) == NULL
    assert h.ltr_listnet_ragged_fwd_bwd(ok, None, ok, None, 3, 8, 0, 1.0, ok, None, None) == NULL
    assert h.ltr_listnet_ragged_fwd_bwd(ok, ok, None, None, 3, 8, 0, 1.0, ok, None, None) == NULL
    assert h.ltr_lambda_ragged_fwd_bwd(ok, ok, None, None, 3, 8, 4, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1.0, ok, ok, None, None) == NULL
    assert h.ltr_lambda_ragged_fwd_bwd(ok, ok, ok, None, 3, 8, 4, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1.0, ok, None, None, None) == NULL
    assert h.ltr_ndcg_at_k_ragged(ok, ok, None, None, 3, 8, 5, 0, 1, 0, ok, None, None) == NULL
    assert h.ltr_ndcg_at_k_ragged(ok, ok, ok, None, 3, 8, 5, 0, 1, 0, None, None, None) == NULL
    # bad enums / scalars
    assert h.ltr_lambda_ragged_fwd_bwd(ok, ok, ok, None, 3, 8, 8, 0, 1.0, 10.0, 1e-10, -1.0, 0, 1.0, ok, ok, None, None) == PARAM
    assert h.ltr_lambda_ragged_fwd_bwd(ok, ok, ok, None, 3, 8, 4, 0, 1.0, 10.0, 1e-10, -1.0, 2, 1.0, ok, ok, None, None) == PARAM
    assert h.ltr_lambda_ragged_fwd_bwd(ok, ok, ok, None, 3, 8, 4, 0, 1.0, 10.0, 0.0, -1.0, 0, 1.0, ok, ok, None, None) == PARAM
    assert h.ltr_ndcg_at_k_ragged(ok, ok, ok, None, 3, 8, 0, 0, 1, 0, ok, None, None) == PARAM
    assert h.ltr_ndcg_at_k_ragged(ok, ok, ok, None, 3, 8, 5, 2, 1, 0, ok, None, None) == PARAM
    # nothing to do is not an error (and launches nothing)
    assert h.ltr_approxndcg_ragged_fwd_bwd(ok, ok, ok, None, 0, 8, 1.0, 1e-10, -1.0, 1.0, ok, None, None) == 0
    assert h.ltr_abi_version() == 1


def test_cpu_tensors_are_refused():
    from ltr_mi355x import LtrDeviceError, ragged
    sl = ragged.RaggedSlates([0, 3, 8])
    s, y = torch.randn(8), torch.randint(0, 5, (8,)).float()
    for call in (lambda: ragged.approx_ndcg(s, y, sl), lambda: ragged.listnet(y, s, sl), lambda: ragged.lambda_loss(s, y, sl),
                 lambda: ragged.lambda_loss(s, y, sl, weighing_scheme="ndcgLoss2PP_scheme", reduction="mean")):
        with pytest.raises(LtrDeviceError):
            call()
    with pytest.raises(ValueError, match="Reduction method"):
        ragged.lambda_loss(s, y, sl, reduction="median")
    with pytest.raises(KeyError):
        ragged.lambda_loss(s, y, sl, weighing_scheme="nope_scheme")


def test_step_ragged_exists_on_both_rankers():
    from ltr_mi355x.linear import LinearFusedRanker
    from ltr_mi355x.scorer import FusedRanker
    assert callable(FusedRanker.step_ragged) and LinearFusedRanker.step_ragged is FusedRanker.step_ragged


# ------------------------------------------------------------------------------- the reference helper is the padded reference
def _padded(s, y, bounds):
    return RC.pad_rectangle(s.double(), bounds, 0.0), RC.pad_rectangle(y.double(), bounds, -1.0)


def test_per_query_loop_equals_padded_oracle_approxndcg():
    bounds = RC.bounds_of(RC.ISSUE_LENGTHS)
    s, y = RC.random_batch(RC.ISSUE_LENGTHS, 41)
    got = RC.oracle_ragged("approxNDCG", s, y, bounds)
    sp, yp = _padded(s, y, bounds)
    sp.requires_grad_(True)
    ref = O.approx_ndcg(sp, yp)
    ref.backward()
    assert abs(float(got["loss"]) - float(ref)) <= 1e-14 * abs(float(ref))
    g = sp.grad
    assert float((RC.unpad(g, bounds) - got["grad"]).abs().max()) <= 1e-15
    mask = yp == -1.0
    assert float(g[mask].abs().max()) == 0.0                       # the gradient on padding is exactly 0


@pytest.mark.parametrize("scheme", O.SCHEMES)
@pytest.mark.parametrize("k", [None, 5])
def test_per_query_loop_equals_padded_oracle_lambda(scheme, k):
    bounds = RC.bounds_of(RC.ISSUE_LENGTHS)
    s, y = RC.random_batch(RC.ISSUE_LENGTHS, 42)
    sp, yp = _padded(s, y, bounds)
    for red in ("sum", "mean"):
        kw = dict(weighing_scheme=scheme, k=k, sigma=1.0, mu=10.0, reduction_log="binary")
        got = RC.oracle_ragged("lambdaLoss", s, y, bounds, reduction=red, **kw)
        x = sp.clone().requires_grad_(True)
        ref = O.lambda_loss(x, yp, RC.EPS, RC.PAD, reduction=red, **kw)
        ref.backward()
        assert abs(float(got["loss"]) - float(ref)) <= 1e-13 * abs(float(ref)), (scheme, k, red)
        top = float(x.grad.abs().max())
        assert float((RC.unpad(x.grad, bounds) - got["grad"]).abs().max()) <= 1e-13 * top
        assert float(x.grad[yp == -1.0].abs().max()) == 0.0


def test_listnet_is_not_the_padded_rectangle():
    """ListNet has no padding mask (listnet.py:5-16): a padded document changes the softmaxes, so only the loop is a reference."""
    bounds = RC.bounds_of([3, 9, 5])
    s, y = RC.random_batch([3, 9, 5], 43)
    got = RC.oracle_ragged("listnet", s, y, bounds)
    sp, yp = _padded(s, y, bounds)
    ref = O.listnet(yp, sp)
    assert abs(float(got["loss"]) - float(ref)) > 1e-3 * abs(float(ref))


def test_band_free_inputs_exist_for_every_tier_length():
    """The clamp-band rule of the GPU lambdaLoss tests (a pair within rounding of a clamp may branch differently in fp32 and fp64):
    every query gets the first ladder rung with an empty band.  Small lengths here; the GPU test asserts it for every length."""
    for S in (1, 2, 3, 16, 17, 64, 129):
        for scheme in ("ndcgLoss2PP_scheme", "rankNetWeightedByGTDiffPowed_scheme"):
            for opt in LT.REQUIRED_OPTS:
                s, y, rung = RC.band_free_query(S, scheme, opt)
                assert s.shape == (S,) and rung in LT.LADDER
