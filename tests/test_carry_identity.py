"""CPU check of the byte-SWAR formulations used by vt_scan_carry_kernel,
vt_scan_carry_col_kernel and vt_scan_generic_kernel
(pyratslam_amd/csrc/view_templates.hip): a NumPy emulation of the stored dword
layout (4 columns per dword, columns >= W and rows >= H zero), the query form
c = -Q mod 256 split into (cL, cH) with padded bytes 0, carry_pair =
popcount(maj(aH, cH, aL + cL)), the sliding byte sums A[o], score(o) = A[o] +
qsum - 256 cnt[o] in uint32 arithmetic, the 8-lane column reduction of the
carry_col form, and wrapped_pair = bytesum((aL + cL) ^ aH ^ cH) of the generic
form must reproduce the oracle's wrapped score (view_templates.py:16-28)
exactly, padding included (W % 4 != 0, W < 4, WD < 8, WD > 8)."""
import numpy as np
import pytest

from oracle import view_templates as V

M = 8
NO = 2 * M - 1
U32 = np.uint64(0xFFFFFFFF)            # dwords are kept in uint64 and masked: mod 2^32
LO, HI = np.uint64(0x7F7F7F7F), np.uint64(0x80808080)


def pack(b, rows):
    """(H, W) byte values -> (rows, WD) dwords, byte k of dword c = column 4c + k;
    columns >= W and rows >= H are zero (vt_store_kernel, vt_qform_kernel)."""
    H, W = b.shape
    WD = (W + 3) // 4
    p = np.zeros((rows, 4 * WD), np.uint64)
    p[:H, :W] = b
    p = p.reshape(rows, WD, 4)
    return p[..., 0] | (p[..., 1] << np.uint64(8)) | (p[..., 2] << np.uint64(16)) | (p[..., 3] << np.uint64(24))


def stored(t):
    """The library's dwords of one template: rows padded to 4 * HQ."""
    return pack(t.astype(np.uint64), 4 * ((t.shape[0] + 3) // 4))


def query_form(q):
    """(cL, cH) per (row, dword column) and qsum = byte sum of c over rows [M, H-M)."""
    H = q.shape[0]
    neg = (256 - q.astype(np.int64)) & 0xFF         # real columns only: a padded byte is 0
    d = pack(neg.astype(np.uint64), H)
    return d & LO, d & HI, np.uint64(bytesum(d[M:H - M]).sum()) & U32


def bytesum(x):
    """v_sad_u8(x, 0, 0): the sum of the four bytes of every dword."""
    return sum((x >> np.uint64(8 * k)) & np.uint64(0xFF) for k in range(4))


def popcount(x):
    b = np.ascontiguousarray(x.astype('<u4')).view(np.uint8)
    return np.unpackbits(b).reshape(x.shape + (32,)).sum(axis=-1).astype(np.uint64)


def bitop3(a, b, c, table):
    """v_bitop3_b32: result bit = table bit (a << 2 | b << 1 | c), bitwise."""
    out = np.zeros_like(a)
    for i in range(8):
        if table >> i & 1:
            out |= (a if i & 4 else ~a) & (b if i & 2 else ~b) & (c if i & 1 else ~c)
    return out & U32


def carry_terms(t, q):
    """Per dword column c and offset index o: the sliding byte sum A[c][o] of the
    template rows [M + o - (M-1), H - M + o - (M-1)) and the carry count cnt[c][o]."""
    H = q.shape[0]
    R0, R1 = M, H - M
    w = stored(t)
    aL, aH, bs = w & LO, w & HI, bytesum(w)
    fx, fy, qsum = query_form(q)
    WD = w.shape[1]
    A = np.zeros((WD, NO), np.uint64)
    cnt = np.zeros((WD, NO), np.uint64)
    win = bs[R0 - (M - 1):R1 - (M - 1)].sum(axis=0) & U32
    A[:, 0] = win
    for o in range(1, NO):
        win = (win + bs[R1 - (M - 1) + o - 1] - bs[R0 - (M - 1) + o - 1]) & U32
        A[:, o] = win
    for o in range(NO):
        s0, s1 = R0 + o - (M - 1), R1 + o - (M - 1)
        cnt[:, o] = popcount(bitop3(aH[s0:s1], fy[R0:R1], (aL[s0:s1] + fx[R0:R1]) & U32, 0xE8)).sum(axis=0)
    return A, cnt, qsum


def carry_score(t, q):
    """vt_scan_carry_kernel: A and cnt summed over the columns, one score per offset."""
    A, cnt, qsum = carry_terms(t, q)
    sc = (A.sum(axis=0) + qsum - np.uint64(256) * cnt.sum(axis=0)) & U32
    return sc.min()


def carry_col_score(t, q):
    """vt_scan_carry_col_kernel: lane cl of 8 sums A - 256 cnt over its columns
    c = cl, cl + 8, ... (nothing when cl >= WD), the lanes meet in a 3-step xor
    butterfly, qsum is added last."""
    A, cnt, qsum = carry_terms(t, q)
    val = np.zeros((8, NO), np.uint64)
    for c in range(A.shape[0]):
        val[c % 8] = (val[c % 8] + A[c] - np.uint64(256) * cnt[c]) & U32
    for step in (1, 2, 4):
        val = (val + val[np.arange(8) ^ step]) & U32
    assert (val == val[0]).all()
    return ((val[0] + qsum) & U32).min()


def generic_score(t, q):
    """vt_scan_generic_kernel: wrapped_pair accumulated over rows [M, H-M) and the
    dword columns, per offset; the minimum over the offsets."""
    H = q.shape[0]
    w = stored(t)
    aL, aH = w & LO, w & HI
    fx, fy, _ = query_form(q)
    best = U32
    for o in range(-(M - 1), M):
        d = bitop3((aL[M + o:H - M + o] + fx[M:H - M]) & U32, aH[M + o:H - M + o], fy[M:H - M], 0x96)
        best = min(best, np.uint64(bytesum(d).sum()) & U32)
    return best


def _case(shape):
    H, W = shape
    rng = np.random.default_rng(100 * H + W)
    lib = rng.integers(0, 256, (3, H, W), dtype=np.uint8)
    lib[1] = np.where(rng.random((H, W)) < 0.5, 0, 255).astype(np.uint8)   # extremes
    lib[2] = 255
    queries = [rng.integers(0, 256, (H, W), dtype=np.uint8), np.roll(lib[0], 3, axis=0),
               np.zeros((H, W), np.uint8), np.full((H, W), 255, np.uint8)]
    return lib, queries


CARRY_SHAPES = [(32, 20), (32, 30), (64, 3), (64, 48)]


@pytest.mark.parametrize('form', [carry_score, carry_col_score])
@pytest.mark.parametrize('shape', CARRY_SHAPES)
def test_carry_scores_equal_wrapped_scores(shape, form):
    lib, queries = _case(shape)
    for q in queries:
        got = np.array([form(t, q) for t in lib], dtype=np.uint64)
        assert np.array_equal(got, V.vt_scores_library(lib, q))


@pytest.mark.parametrize('shape', CARRY_SHAPES + [(18, 8), (40, 32)])
def test_generic_scores_equal_wrapped_scores(shape):
    lib, queries = _case(shape)
    for q in queries:
        got = np.array([generic_score(t, q) for t in lib], dtype=np.uint64)
        assert np.array_equal(got, V.vt_scores_library(lib, q))
