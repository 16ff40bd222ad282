"""CPU: the host side of the fixed-length-slate path (ltr_mi355x/slates.py, csrc/ltr_data.hip ltr_slates_*) -- the selection rule as
restated in tests/slate_build_cases.py, its uniformity, the launchers' argument contract (answered before any launch) and the host
fields of FixedSlates.  The device is held to the restatement in tests/test_slate_build_gpu.py."""
import ctypes

import numpy as np
import pytest
import torch

import slate_build_cases as SC


@pytest.fixture(scope="module")
def handle():
    from ltr_mi355x.build import build
    build(force=False, verbose=False)
    import ltr_mi355x
    return ltr_mi355x.lib()


# ---------------------------------------------------------------------------------------------------- 1. the restatement
@pytest.mark.parametrize("mode", [SC.FIRST, SC.SAMPLE])
def test_restatement_keeps_min_len_S_distinct_rows_ascending(mode):
    offsets = SC.bounds_of(SC.SELECT_LENGTHS)
    for S in SC.SELECT_S:
        rows, mask = SC.select_host(offsets, S, mode, 12345)
        for q, n in enumerate(SC.SELECT_LENGTHS):
            k = min(n, S)
            real = rows[q, :k]
            assert (np.diff(real) > 0).all(), (S, q)                               # ascending, hence distinct
            assert real.min() >= offsets[q] and real.max() < offsets[q + 1]        # the query's own rows
            assert (rows[q, k:] == -1).all() and (mask[q, :k] == 0).all() and (mask[q, k:] == 1).all()
            if mode == SC.FIRST or n <= S:
                assert np.array_equal(real, offsets[q] + np.arange(k))


def test_sample_of_a_short_query_is_first_and_seeds_differ():
    offsets = SC.bounds_of(SC.SELECT_LENGTHS)
    a, _ = SC.select_host(offsets, 100, SC.SAMPLE, 1)
    b, _ = SC.select_host(offsets, 100, SC.SAMPLE, 2)
    f, _ = SC.select_host(offsets, 100, SC.FIRST, 1)
    for q, n in enumerate(SC.SELECT_LENGTHS):
        if n <= 100:
            assert np.array_equal(a[q], f[q]) and np.array_equal(b[q], f[q])
        else:
            assert not np.array_equal(a[q], b[q]) and not np.array_equal(a[q], f[q])
    # the query id is part of the key: two queries of one length draw different subsets under one seed
    assert not np.array_equal(SC.kept_docs(300, 100, SC.SAMPLE, 1, 4), SC.kept_docs(300, 100, SC.SAMPLE, 1, 5))
    # a length outside 1 .. 2048 keeps nothing
    assert SC.kept_docs(0, 5, SC.SAMPLE, 1, 0).size == 0 and SC.kept_docs(2049, 5, SC.FIRST, 1, 0).size == 0


def test_key_fixed_vector():
    """key(seed=1, q=2, j=3) in Python integers, written out step by step here, against both statements in slate_build_cases."""
    m = (1 << 64) - 1
    z = 1 ^ ((2 * 0xD1B54A32D192ED03 + 3 * 0x9E3779B97F4A7C15 + 0x8CB92BA72F3D8DD7) % (1 << 64))
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    want = z ^ (z >> 31)
    assert SC.key_int(1, 2, 3) == want
    assert int(SC.keys(1, 2, 8)[3]) == want
    for seed, q in ((0, 0), (SC.SEEDS[1], 16), ((1 << 64) - 1, 2 ** 31 - 1)):
        assert [int(v) for v in SC.keys(seed, q, 70)] == [SC.key_int(seed, q, j) for j in range(70)]


# ---------------------------------------------------------------------------------------------------- 2. uniformity
def test_sampling_rule_is_uniform():
    """len 12, S 5, seeds 0 .. 3999, q 7: every document's inclusion count within 5 sigma of 4000 * 5 / 12 = 1666.7, sigma =
    sqrt(4000 * (5 / 12) * (7 / 12)) = 31.2 -> 1667 +- 156.  Deterministic: a miss means the hash is not the stated one."""
    counts = np.zeros(12, dtype=np.int64)
    for seed in range(4000):
        counts[SC.kept_docs(12, 5, SC.SAMPLE, seed, 7)] += 1
    print("inclusion counts", counts.tolist())
    assert counts.sum() == 4000 * 5
    assert (np.abs(counts - 1667) <= 156).all(), counts


# ---------------------------------------------------------------------------------------------------- 3. argument rejection
_PTR = object()
_SIGNATURES = {
    "ltr_slates_select": [("offsets", _PTR), ("queries", _PTR), ("n_queries", 2), ("S", 8), ("mode", 0), ("seed", 1), ("rows", _PTR),
                          ("mask", _PTR)],
    "ltr_slates_gather_f32": [("src", _PTR), ("src_rows", 4), ("rows", _PTR), ("n_slots", 4), ("row_floats", 4), ("fill", 0.0),
                              ("dst", _PTR)],
    "ltr_slates_scatter_f32": [("src", _PTR), ("rows", _PTR), ("n_slots", 4), ("row_floats", 4), ("dst_rows", 4), ("dst", _PTR)],
    "ltr_slates_build": [("X", _PTR), ("y", _PTR), ("offsets", _PTR), ("queries", _PTR), ("n_queries", 2), ("S", 8), ("F", 4),
                         ("mode", 1), ("seed", 1), ("pad", -1.0), ("X_out", _PTR), ("y_out", _PTR), ("mask", _PTR), ("rows", _PTR)],
}
# (arguments changed from the valid call, code): -1 LTR_ERR_NULL, -2 LTR_ERR_SHAPE, -3 LTR_ERR_PARAM, 0 the zero-size call.  Every
# row is answered before any launch: NULL first, then shapes, then the mode, then the empty call (the order of the loss launchers).
_CONTRACT = {
    "ltr_slates_select": [
        ({"offsets": None}, -1), ({"rows": None}, -1), ({"n_queries": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2), ({"mode": 2}, -3),
        ({"mode": -1}, -3), ({"n_queries": 0}, 0), ({"n_queries": 0, "mask": None, "queries": None}, 0), ({"rows": None, "S": 0}, -1),
        ({"S": 0, "mode": 2}, -2), ({"mode": 2, "n_queries": 0}, -3), ({"S": 0, "n_queries": 0}, -2),
    ],
    "ltr_slates_gather_f32": [
        ({"src": None}, -1), ({"rows": None}, -1), ({"dst": None}, -1), ({"n_slots": -1}, -2), ({"src_rows": -1}, -2),
        ({"row_floats": 0}, -2), ({"n_slots": 0}, 0), ({"dst": None, "row_floats": 0}, -1), ({"row_floats": 0, "n_slots": 0}, -2),
    ],
    "ltr_slates_scatter_f32": [
        ({"src": None}, -1), ({"rows": None}, -1), ({"dst": None}, -1), ({"n_slots": -1}, -2), ({"dst_rows": -1}, -2),
        ({"row_floats": 0}, -2), ({"n_slots": 0}, 0), ({"dst": None, "row_floats": 0}, -1), ({"row_floats": 0, "n_slots": 0}, -2),
    ],
    "ltr_slates_build": [
        ({"X": None}, -1), ({"y": None}, -1), ({"offsets": None}, -1), ({"X_out": None}, -1), ({"y_out": None}, -1),
        ({"n_queries": -1}, -2), ({"S": 0}, -2), ({"S": 2049}, -2), ({"F": 0}, -2), ({"mode": 2}, -3), ({"mode": -1}, -3),
        ({"n_queries": 0}, 0), ({"n_queries": 0, "mask": None, "rows": None, "queries": None}, 0), ({"y_out": None, "F": 0}, -1),
        ({"F": 0, "mode": 2}, -2), ({"mode": 2, "n_queries": 0}, -3), ({"S": 2049, "n_queries": 0}, -2),
    ],
}
_SCRATCH = (ctypes.c_char * 64)()


@pytest.mark.parametrize("name", sorted(_CONTRACT))
def test_launchers_answer_before_any_launch(handle, name):
    sig = _SIGNATURES[name]
    for changed, code in _CONTRACT[name]:
        assert set(changed) <= {n for n, _ in sig}, (name, changed)
        args = [changed.get(n, v) for n, v in sig]
        got = getattr(handle, name)(*[ctypes.addressof(_SCRATCH) if a is _PTR else a for a in args], None)
        assert got == code, (name, changed, got)


# ---------------------------------------------------------------------------------------------------- 4. / 5. host layer
def test_fixed_slates_host_fields():
    from ltr_mi355x.ragged import RaggedSlates
    from ltr_mi355x.slates import FixedSlates
    slates = RaggedSlates(SC.bounds_of([3, 100, 101, 1, 2048, 99]))
    f = FixedSlates(slates, 100, None, None)
    assert f.S == 100 and f.n_docs == 2352 and f.n_queries == 6
    assert f.kept.tolist() == [3, 100, 100, 1, 100, 99] and f.truncated is True
    g = FixedSlates(slates, 2048, None, None)
    assert g.kept.tolist() == [3, 100, 101, 1, 2048, 99] and g.truncated is False
    assert FixedSlates(RaggedSlates(SC.bounds_of([])), 7, None, None).truncated is False
    assert hasattr(RaggedSlates, "fixed_length")


def test_cpu_tensors_and_bad_arguments_are_refused():
    from ltr_mi355x import LtrDeviceError
    from ltr_mi355x.ragged import RaggedSlates
    from ltr_mi355x.slates import FixedSlates, fixed_length, from_slates, to_slates
    lengths = [3, 9, 4]
    slates = RaggedSlates(SC.bounds_of(lengths))
    X, y = SC.batch(lengths, 8, 0)
    with pytest.raises(LtrDeviceError):
        to_slates(X, y, slates, 4)
    with pytest.raises(LtrDeviceError):
        fixed_length(slates, 4)                        # host-only slates: nothing to launch on
    with pytest.raises(LtrDeviceError):
        slates.fixed_length(4, mode="sample", seed=3)
    rows, _ = SC.select_host(slates.offsets_host, 4, SC.FIRST, 0)
    f = FixedSlates(slates, 4, torch.as_tensor(rows), None)
    with pytest.raises(LtrDeviceError):
        f.gather(y)
    with pytest.raises(LtrDeviceError):
        f.scatter(torch.zeros(3, 4))
    with pytest.raises(LtrDeviceError):
        from_slates(torch.zeros(3, 4), f)
    for S in (0, 2049):
        with pytest.raises(ValueError, match="slate length"):
            to_slates(X, y, slates, S)
    with pytest.raises(ValueError, match="mode"):
        fixed_length(slates, 4, mode="random")
