"""Helpers shared by tests/test_slate_build_cpu.py and tests/test_slate_build_gpu.py (a plain module, no fixtures): the host
restatement of ltr_slates_select in numpy uint64 (include/ltr_mi355x.h states the rule), and the case builders.

select_host is the definition the device is held to, bit for bit: per listed query the kept documents (the first S, or the S smallest
64-bit keys with ties to the lower index), in ascending document order, padding behind them."""
import numpy as np
import torch

FIRST, SAMPLE = 0, 1
MODES = {"first": FIRST, "sample": SAMPLE}
MAX_SLATE = 2048
SELECT_LENGTHS = (1, 2, 4, 5, 6, 31, 32, 33, 99, 100, 101, 255, 256, 257, 1000, 2047, 2048)
SELECT_S = (1, 5, 32, 100, 2048)
SEEDS = (0, 0x9E3779B97F4A7C15)                       # a small one and one with high bits set

_Q, _J, _C = 0xD1B54A32D192ED03, 0x9E3779B97F4A7C15, 0x8CB92BA72F3D8DD7
_M1, _M2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
_MASK = (1 << 64) - 1


def key_int(seed, q, j):
    """The key of local document j of query q in Python integers (arbitrary precision, reduced mod 2^64 by hand)."""
    z = (seed ^ ((q * _Q + j * _J + _C) & _MASK)) & _MASK
    z = ((z ^ (z >> 30)) * _M1) & _MASK
    z = ((z ^ (z >> 27)) * _M2) & _MASK
    return z ^ (z >> 31)


def keys(seed, q, n):
    """Keys of local documents 0 .. n - 1 of query q: numpy uint64, wrapping arithmetic."""
    u = np.uint64
    with np.errstate(over="ignore"):
        j = np.arange(n, dtype=np.uint64)
        z = u(seed & _MASK) ^ (np.full(n, q, dtype=np.uint64) * u(_Q) + j * u(_J) + u(_C))
        z = (z ^ (z >> u(30))) * u(_M1)
        z = (z ^ (z >> u(27))) * u(_M2)
        return z ^ (z >> u(31))


def kept_docs(length, S, mode, seed, q):
    """Ascending local indices of the documents query q keeps."""
    if not 1 <= length <= MAX_SLATE:
        return np.zeros(0, dtype=np.int64)
    if mode == FIRST or length <= S:
        return np.arange(min(length, S), dtype=np.int64)
    order = np.argsort(keys(seed, q, length), kind="stable")          # stable: ties to the lower index
    return np.sort(order[:S]).astype(np.int64)


def select_host(offsets, S, mode, seed, queries=None):
    """(rows [n, S] int64, mask [n, S] uint8) of the listed queries (None: all), as ltr_slates_select writes them."""
    offsets = np.asarray(offsets, dtype=np.int64)
    listed = np.arange(offsets.size - 1) if queries is None else np.asarray(queries)
    rows = np.full((listed.size, S), -1, dtype=np.int64)
    for i, q in enumerate(listed):
        keep = kept_docs(int(offsets[q + 1] - offsets[q]), S, mode, seed, int(q))
        rows[i, :keep.size] = offsets[q] + keep
    return rows, (rows < 0).astype(np.uint8)


def bounds_of(lengths):
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


def batch(lengths, F, seed):
    """(X [n_docs, F], y [n_docs]) fp32: randn features, integer grades 0 .. 4."""
    g = torch.Generator().manual_seed(seed)
    n = int(sum(lengths))
    return torch.randn(n, F, generator=g), torch.randint(0, 5, (n,), generator=g).float()


def special_payload(n, row, seed):
    """[n, row] fp32 whose first entries per row cycle through NaNs with payloads, +-inf and -0.0 (compared as int32 bits)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randn(n, row, generator=g)
    bits = torch.tensor([0x7FC00001, -0x00400000 + 0x123, 0x7F800000, -0x00800000, -0x80000000, 0x7F800001], dtype=torch.int32)
    flat = t.view(-1)
    idx = torch.arange(0, flat.numel(), 3)
    flat.view(torch.int32)[idx] = bits[torch.arange(idx.numel()) % bits.numel()]
    return t


def pad_host(v, rows, fill):
    """v [n_docs, ...] -> [B, S, ...] by the row map, `fill` where rows < 0: the torch-indexing statement of gather, on the CPU."""
    rows = torch.as_tensor(rows)
    out = v[rows.clamp(min=0)].clone()
    out[rows < 0] = fill
    return out
