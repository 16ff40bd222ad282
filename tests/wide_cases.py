"""Cases shared by tests/test_wide_cpu.py and tests/test_wide_gpu.py (FC scorers wider than 136 features, csrc/ltr_wide.hip).

The sizes at which ltr_gemm_f32 takes another path, as csrc/ltr_wide.hip fixes them:
    TILE_M = TILE_N = 64    output tile of one workgroup (rows and columns past the extents are zero-filled in LDS)
    TILE_K = 16             k tile staged through LDS; a split over K cuts in multiples of it
    QUAD   = 4              floats of one 16-byte load: an operand is read that way when its base is 16-byte aligned and its leading
                            dimension a multiple of 4 (the last, partial quad of a row element by element), else 4 bytes at a time
    sub-tiles: a wave owns a 32 x 32 quarter as 2 x 2 MFMA tiles of 16 x 16 -- 15 / 17 / 31 / 33 sit inside the widths below.
"""
import numpy as np

TILE_M = TILE_N = 64
TILE_K = 16
QUAD = 4
FORMS = {"forward": (0, 0), "dh": (0, 1), "dW": (1, 1)}       # (a_kmajor, b_kmajor) of include/ltr_mi355x.h


def _case(form, M, N, K, pad_a=0, pad_b=0, off_a=0, off_b=0, splits=1):
    """pad_*: extra floats on the operand's leading dimension; off_*: floats the operand's base is moved off a 16-byte boundary."""
    return dict(form=form, M=M, N=N, K=K, pad_a=pad_a, pad_b=pad_b, off_a=off_a, off_b=off_b, splits=splits)


def gemm_cases():
    cases = []
    for form in FORMS:
        # every extent one below, at and one above its tile, one at a time, then all three above
        for M, N, K in [(63, 64, 16), (64, 64, 16), (65, 64, 16), (64, 63, 16), (64, 65, 16), (64, 64, 15), (64, 64, 17), (65, 65, 17),
                        (129, 127, 33)]:
            cases.append(_case(form, M, N, K))
        # 16-byte path with a partial last quad (leading dimension padded to a multiple of 4) and the 4-byte path by the base alone
        cases.append(_case(form, 65, 65, 17, pad_a=3, pad_b=3))
        cases.append(_case(form, 64, 64, 32, off_a=1))
        cases.append(_case(form, 64, 64, 32, off_b=1))
    # M = 1 and the collections' widths (137 = the first width past the slate pipeline, Istella 220, Yahoo's 519 in use, the limit 1024)
    for W in (137, 220, 519, 1024):
        cases.append(_case("forward", 1, W, W))
        cases.append(_case("forward", 37, W, W))
        cases.append(_case("dh", 37, W, W))
        cases.append(_case("dW", W if W < 1024 else 40, W, 185))
    cases.append(_case("dW", 32, 1024, 70))
    # split over K: 1 and 3 slices, a short last slice (185 = 12 k tiles -> 64 + 64 + 57), more slices than k tiles (40 -> 16 + 16 + 8
    # and two empty slices, which write zeros)
    for form in FORMS:
        cases.append(_case(form, 65, 70, 185, splits=3))
        cases.append(_case(form, 65, 70, 40, splits=5))
    cases.append(_case("dW", 220, 220, 185, splits=3))
    return cases


def case_id(c):
    extra = "".join(f"-{k}{c[k]}" for k in ("pad_a", "pad_b", "off_a", "off_b") if c[k]) + (f"-s{c['splits']}" if c["splits"] > 1 else "")
    return f"{c['form']}-{c['M']}x{c['N']}x{c['K']}{extra}"


def operand_shapes(c):
    """(rows, ld) of A's and B's storage: a k-major operand is stored [K][extent + pad], the other [extent][K + pad]."""
    ak, bk = FORMS[c["form"]]
    a = (c["K"], c["M"] + c["pad_a"]) if ak else (c["M"], c["K"] + c["pad_a"])
    b = (c["K"], c["N"] + c["pad_b"]) if bk else (c["N"], c["K"] + c["pad_b"])
    return a, b


def logical(c, a_store, b_store):
    """The storage arrays -> A [M][K] and B [N][K]."""
    ak, bk = FORMS[c["form"]]
    A = a_store[:, :c["M"]].T if ak else a_store[:, :c["K"]]
    B = b_store[:, :c["N"]].T if bk else b_store[:, :c["K"]]
    return A, B


def gemm_bound(A, B, bias=None):
    """|C - C64| <= (K + 4) 2^-24 (|A| |B|^T + |bias|): the dot-product bound gamma_n for any summation order, fused or not, one more
    rounding for the bias and one for the fp64 -> fp32 store of a split reduce."""
    K = A.shape[1]
    mag = np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)).T
    if bias is not None:
        mag = mag + np.abs(bias.astype(np.float64))[None, :]
    return (K + 4) * 2.0 ** -24 * mag


def r4(n):
    return (n + 3) // 4 * 4


def splits(M, N, n_docs, grid):
    """The slices of a weight-gradient GEMM, as include/ltr_mi355x.h states them."""
    tiles = -(-M // 64) * -(-N // 64)
    return max(1, min(-(-grid // tiles), -(-max(n_docs, 1) // 64), 1024))


def acts_floats(kind, F, H1, H2, n):
    return r4(n * H1) + (r4(n * H2) if kind == 0 else 0)


def ws_floats(kind, F, H1, H2, n, grid):
    parts, hmax, dz = splits(H1, F, n, grid) * H1 * F, H1, r4(n * H1)
    if kind == 0:
        parts, hmax, dz = max(parts, splits(H2, H1, n, grid) * H2 * H1), max(H1, H2), dz + r4(n * H2)
    return dz + r4(max(grid * hmax, parts))
