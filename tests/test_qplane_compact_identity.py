"""CPU check of the compact query planes of the pruned plane scan (vt_qplane_kernel's
compact mode, pyratslam_amd/csrc/view_templates.hip).

Full form: for every start row s in [M-3, H-M-1] = 5..55 and column group cg, the unit of
rows s..s+3 with the rows outside [M, H-M) zeroed; bit b of plane word k is bit k of pixel
(s + b/8, 8 cg + b%8).  Compact form: the units of the aligned start rows S = 5 + 4i,
i < 13, only (rows 5, 9, .., 53), and the unit of start row 57 taken as zero (rows 57..60
are all zeroed).  The identity every reader of the compact form relies on:

    word_k(S + r) = alignbit(word_k(S + 4), word_k(S), 8 r),   r = 0..3

(alignbit(hi, lo, n) = the low 32 bits of (hi:lo) >> n), exactly, borders included."""
import numpy as np
import pytest

from oracle import view_templates as V

M = V.MAX_OFFSET
H, W, CG = 64, 32, 4
S0, S1 = M - 3, H - M - 1
NA = 13


def unit_words(img, s):
    """uint32[CG][8]: the plane words of the unit of rows s..s+3 (zeroed outside [M, H-M))."""
    z = np.zeros((H + 8, W), dtype=np.uint32)
    z[M:H - M] = img[M:H - M]
    rows = z[s:s + 4].reshape(4, CG, 8)                                  # [dr][cg][c]
    bits = (rows[..., None] >> np.arange(8, dtype=np.uint32)) & 1       # [dr][cg][c][k]
    sh = (8 * np.arange(4, dtype=np.uint32)[:, None] + np.arange(8, dtype=np.uint32)[None])   # b = 8 dr + c
    return (bits << sh[:, None, :, None]).sum(axis=(0, 2), dtype=np.uint64).astype(np.uint32)


def full_planes(img):
    """What vt_qplane_kernel writes in full mode: uint32[CG][51][8]."""
    return np.stack([unit_words(img, s) for s in range(S0, S1 + 1)], axis=1)


def compact_planes(img):
    """... and in compact mode: uint32[CG][13][8], the aligned start rows."""
    return np.stack([unit_words(img, S0 + 4 * i) for i in range(NA)], axis=1)


def alignbit(hi, lo, n):
    return (((hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)) >> np.uint64(n)).astype(np.uint32)


def expand(compact):
    """Every start row from the compact planes; the unit past the last is zero."""
    ext = np.concatenate([compact, np.zeros_like(compact[:, :1])], axis=1)
    out = np.empty((CG, S1 - S0 + 1, 8), dtype=np.uint32)
    for si in range(S1 - S0 + 1):
        out[:, si] = alignbit(ext[:, si // 4 + 1], ext[:, si // 4], 8 * (si % 4))
    return out


def images():
    rng = np.random.default_rng(211)
    for i in range(4):
        yield 'random%d' % i, rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    yield 'zeros', np.zeros((H, W), dtype=np.uint8)
    yield 'ones', np.full((H, W), 255, dtype=np.uint8)
    for lo in (7, 55):   # one row outside the window and its neighbour inside
        img = np.zeros((H, W), dtype=np.uint8)
        img[lo:lo + 2] = rng.integers(1, 256, size=(2, W), dtype=np.uint8)
        yield 'rows%d_%d' % (lo, lo + 1), img
    img = np.zeros((H, W), dtype=np.uint8)
    img[[7, 8, 55, 56]] = 255
    yield 'borders255', img


def test_the_full_form_is_the_bit_layout_the_scan_reads():
    rng = np.random.default_rng(212)
    img = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    full = full_planes(img)
    for s, cg, k, b in ((5, 0, 0, 0), (5, 3, 7, 31), (8, 1, 3, 9), (30, 2, 5, 17), (55, 3, 0, 7), (55, 0, 7, 8)):
        r, c = s + b // 8, 8 * cg + b % 8
        want = (int(img[r, c]) >> k) & 1 if M <= r < H - M else 0
        assert (int(full[cg, s - S0, k]) >> b) & 1 == want


@pytest.mark.parametrize('name,img', list(images()), ids=[n for n, _ in images()])
def test_funnel_shift_of_two_aligned_units_is_the_full_word(name, img):
    full, comp = full_planes(img), compact_planes(img)
    assert full.shape == (CG, 51, 8) and comp.shape == (CG, NA, 8)
    # start row 57 (the unit past the last aligned one) is all zero
    assert not unit_words(img, S0 + 4 * NA).any()
    got = expand(comp)
    for s in range(S0, S1 + 1):
        for cg in range(CG):
            for k in range(8):
                assert got[cg, s - S0, k] == full[cg, s - S0, k], (name, s, cg, k)
    if name == 'ones':
        assert full[0, 0, 0] == 0xFF000000 and full[0, S1 - S0, 0] == 0x000000FF
