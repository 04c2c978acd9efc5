"""Host logic: the one-MFMA image of an edge table (packing._etab_frag1) holds T_hi twice and T_lo once in the k-slots the
kernel's operand e_hi | e_lo | e_hi | 0 meets (csrc/pf_mfma.h pf_edge_operand / pf_mm1).  CPU only."""
import numpy as np
import pytest

from puflow_amd.packing import (_ETAB_COLS, _etab_dense, _etab_frag1, ec1n_unit0_table, etab_unpack_frag1, f16n_scale,
                                fold_state_dict, pack_plan)
from puflow_amd.weights import synth_state_dict


def _random_table(rows, seed, with_norm):
    rng = np.random.default_rng(seed)
    t = _etab_dense(rng.standard_normal((rows, 3)), rng.standard_normal((rows, 3)),
                    rng.standard_normal(rows) if with_norm else None, rng.standard_normal(rows))
    return (t.astype(np.float64) * f16n_scale(t)).astype(np.float32)             # scaled as pack_plan scales a group


def _unit0_table():
    return ec1n_unit0_table(fold_state_dict(synth_state_dict(2021))["units"][0])[0]         # as pack_plan packs it


TABLES = [("random64", lambda: _random_table(64, 0, True)), ("random128", lambda: _random_table(128, 1, False)),
          ("ragged40", lambda: _random_table(40, 2, True)), ("unit0", _unit0_table)]


@pytest.fixture(scope="module", params=TABLES, ids=[n for n, _ in TABLES])
def table(request):
    T = np.asarray(request.param[1](), dtype=np.float32)
    return T, _etab_frag1(T)


def test_image_size_and_layout(table):
    T, F = table
    rows = T.shape[0]
    assert F.dtype == np.float32 and F.size == ((rows + 15) // 16) * 256          # one 1-KiB fragment per 16 rows
    # lane l = 16 q + row, slot j of fragment ob  <->  T[16 ob + row][_ETAB_COLS[j]]: hi for q = 0, 1, lo for q = 2
    h = F.view(np.float16).reshape(-1, 64, 8)
    ob, row, j = rows // 16 - 1, 5, 6
    want = np.float16(T[16 * ob + row, _ETAB_COLS[j]])
    assert h[ob, 16 * 0 + row, j] == want and h[ob, 16 * 1 + row, j] == want
    assert h[ob, 16 * 2 + row, j] == np.float16(T[16 * ob + row, _ETAB_COLS[j]] - np.float32(want))


def test_hi_plus_lo_reproduces_the_table(table):
    """T_hi + T_lo against the float64 table, 2^-21 relative, element by element.  A natural-scale low half is an fp16
    subnormal once |T| < 2^-4 (absolute floor 2^-25), which is why every table is stored times a power of two that puts its
    largest entry into [2^13, 2^14) - unit 0's included (packing.ec1n_unit0_table; without it 2 of its 448 entries,
    |T| < 0.02, sat at 1.6e-6)."""
    T, F = table
    hi0, hi1, lo, rest = etab_unpack_frag1(F, T.shape[0])
    ref = T.astype(np.float64)[:, _ETAB_COLS]
    np.testing.assert_array_equal(hi0, hi1)                                        # the two hi copies are identical
    assert np.all(rest == 0)                                                       # q = 3: every other k-slot is zero
    err = np.abs(hi0 + lo - ref)
    assert np.all(err <= np.abs(ref) * 2.0 ** -21)
    # rows past the table (the last fragment's padding) are zero too
    full = F.view(np.float16).reshape(-1, 4, 16, 8)
    pad = (-T.shape[0]) % 16
    if pad:
        assert np.all(full[-1, :, 16 - pad:, :] == 0)


def test_one_mfma_sums_the_three_split_terms(table):
    """The MFMA as the kernel issues it: A = the image (lane 16 q + row: k-slots 8 q .. 8 q + 7), B = e_hi | e_lo | e_hi | 0 over
    q = 0..3.  Its sum over the 32 k-slots is the split product T_hi e_hi + T_hi e_lo + T_lo e_hi: T e to fp32 rounding."""
    T, F = table
    rows = T.shape[0]
    rng = np.random.default_rng(7)
    e = rng.uniform(-1, 1, (8, 16)).astype(np.float32)                             # 16 edge columns
    e[7] = 1.0
    e_hi = e.astype(np.float16)
    e_lo = (e - e_hi.astype(np.float32)).astype(np.float16)
    Bop = np.concatenate([e_hi, e_lo, e_hi, np.zeros_like(e_hi)]).astype(np.float64)          # [32 k-slots, 16]
    A = F.view(np.float16).reshape(-1, 4, 16, 8).transpose(0, 2, 1, 3).reshape(-1, 32).astype(np.float64)[:rows]   # [rows, 32 k-slots]
    got = A @ Bop
    ref = T.astype(np.float64)[:, _ETAB_COLS] @ e.astype(np.float64)
    scale = np.abs(T.astype(np.float64)[:, _ETAB_COLS]) @ np.abs(e.astype(np.float64))
    assert np.all(np.abs(got - ref) <= scale * 2.0 ** -20)
    hi0, _, lo, _ = etab_unpack_frag1(F, rows)
    three = hi0 @ e_hi.astype(np.float64) + hi0 @ e_lo.astype(np.float64) + lo @ e_hi.astype(np.float64)
    np.testing.assert_allclose(got, three, rtol=0, atol=1e-9 * float(scale.max()))


def test_unit0_image_in_the_blob_carries_its_scale():
    """pack_plan: behind unit 0's growth fragments lie the table's one-MFMA image and then 2^-sw, the power of two the kernel
    multiplies the table products by; image times 2^-sw is the unscaled table."""
    plan = fold_state_dict(synth_state_dict(2021))
    pk = pack_plan(plan)
    T, inv = ec1n_unit0_table(plan["units"][0])
    o = pk["ec1n_w"][0] + (4 + 2 * 2) * 512                                        # G1 | G2 | G3 (4 pairs), Gout (2 x 2 pairs)
    img = pk["blob"][o:o + 6 * 256]
    np.testing.assert_array_equal(img, _etab_frag1(T))
    assert pk["blob"][o + 6 * 256] == inv and np.log2(float(inv)) == np.round(np.log2(float(inv)))
    assert 2.0 ** 13 <= np.abs(T).max() < 2.0 ** 14
    hi0, _, lo, _ = etab_unpack_frag1(img, 96)
    u = plan["units"][0]
    raw = np.concatenate([u["PA"], u["QB"][:, :1], u["QB"][:, 1:], np.zeros((96, 1)), u["pb"][:, None]], axis=1)
    a = np.repeat(4.0 ** np.arange(5), [16, 16, 16, 16, 32])[:, None]             # ec4_scales(4, 16, 32): the rows' activation scales
    np.testing.assert_allclose((hi0 + lo) * float(inv), raw * a, rtol=2.0 ** -21, atol=0)


def test_rejects_a_matrix_that_is_no_edge_table():
    W = np.zeros((16, 32), np.float32)
    W[3, 7] = 1.0
    with pytest.raises(ValueError):
        _etab_frag1(W)
