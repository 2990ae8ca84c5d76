"""The cases of the direct tests of the training products (tests/test_gpu_train_products.py) and their premises
(tests/test_train_product_premises.py checks them without a device): the shapes, the routing constants of csrc/hip/train.hip,
csrc/hip/conv1d_grad.hip, csrc/hip/conv1d.hip and csrc/host/train.c / conv_1d.c that decide which kernel a shape takes, one predicate
per entry point that restates those conditions, the inputs and the int64 references.  A helper, no test.

The method is integers: every input is drawn from -3 .. 3 and stored as f32.  Every product and every partial sum is then an integer
far below 2^24, so the f32 result is exact in ANY summation order, fused or not; small integers are exact in bf16 too, so the same holds
on the bf16 x 3 split path (the middle and low images are zero).  The expected value is an int64 computation of the definition and the
comparison is equality.  exact_cap() is the premise: 9 * terms + |initial C| < 2^24 for every case."""
import ctypes as C
import functools

import numpy as np

# ---- mirrored from the sources; test_train_product_premises.py reads them back out of the files and fails when they drift ----------
MFMA_MACS = 1 << 27                                 # train.hip nntk_outer_mfma_launch, train.c NNTK_TRAIN_MFMA_MACS, conv_1d.c conv_gradient_dev
OUTER_TILE = 128                                    # train.hip: a workgroup's output tile, four waves of 64 x 64
OUTER_SLICES = 32                                   # train.hip: row slices of the VALU forms, and the most the MFMA forms take
OUTER_WORKGROUPS = 768                              # train.hip nntk_outer_mfma_launch: (tile, slice) workgroups aimed at
OUTER_SLICE_MIN_ROWS = 64                           # ... and at least this many rows a slice
OUTER_TRIP_ROWS = 8                                 # four row pairs per trip of the MFMA loops
OUTER_MIN_I, OUTER_MIN_K = 32, 32                   # train.hip nntk_outer_mfma_launch
GRAD_SLICES = 32                                    # conv1d_grad.hip
COLMAT_CHUNKS = 8                                   # train.hip rows_times_colmat_kernel (out of scope here, mirrored for the record)
GEMM_MIN_K, GEMM_MIN_I = 16, 32                     # train.c nntk_train_rows_times_rowmat
DX_MIN_CIN, DX_MIN_COUT = 32, 16                    # conv_1d.c conv_gradient_dev
CONV_BM, CONV_KC = 128, 16                          # conv1d_kernels.hpp
CONV_VALU_KDIM, CONV_VALU_COUT = 16, 32             # conv1d.hip nntk_shim_conv1d: below either, conv1d_valu_kernel
PLAIN_BYTES = 2.0e9                                 # train.hip: the plain kernel's 32-bit buffer range

VALU, COLSUM = "outer_partial_kernel", "colsum_partial_kernel"
PLAIN, PLAIN_SHIFT, GENERAL = "outer_mfma_plain_kernel<false>", "outer_mfma_plain_kernel<true>", "outer_mfma_kernel"
CONV_DW_VALU = "conv1d_dw_partial_kernel"
CONV_VALU, CONV_EXACT, CONV_SPLIT = "conv1d_valu_kernel", "conv1d_mfma_kernel", "conv1d_mfma_bf16x3_kernel"

LO, HI = -3, 3                                      # the integers every input is drawn from
C0 = 50                                             # C and c start from integers in -C0 .. C0
EXACT = 1 << 24


def outer_slices(rows, I, K):
    """the slice formula of nntk_outer_mfma_launch"""
    ti, tk = (I + OUTER_TILE - 1) // OUTER_TILE, (K + OUTER_TILE - 1) // OUTER_TILE
    slices = (OUTER_WORKGROUPS + ti * tk - 1) // (ti * tk)
    slices = min(slices, OUTER_SLICES)
    slices = min(slices, rows // OUTER_SLICE_MIN_ROWS)
    return max(slices, 1)


def outer_route(rows, I, K, a_shift_T, rps=None, row_pitch=None, plain_option=1):
    """(kernel, slices) of C += A^T B: nntk_shim_outer_accumulate (rps = rows, row_pitch = I) or, with rps / row_pitch given, the
    im2col view nntk_shim_conv1d_grad passes to nntk_outer_mfma_launch"""
    rps = rows if rps is None else rps
    row_pitch = I if row_pitch is None else row_pitch
    if I == 0:
        return COLSUM, OUTER_SLICES
    if not (I >= OUTER_MIN_I and K >= OUTER_MIN_K and rps >= 1 and float(rows) * I * K >= float(MFMA_MACS)):
        return VALU, OUTER_SLICES
    slices = outer_slices(rows, I, K)
    plain = rps >= rows and row_pitch == I and float(rows // slices + 2) * max(I, K) * 4 < PLAIN_BYTES and plain_option != 0
    return (PLAIN_SHIFT if a_shift_T > 0 else PLAIN) if plain else GENERAL, slices


def slice_starts(rows, slices):
    """r0 of every slice: rows * z / slices, as every sliced kernel cuts them"""
    return [rows * z // slices for z in range(slices + 1)]


def conv_a4(Cin, aligned=True, conv_a4_option=1):
    """16-byte window loads: always at the option's default (pieces past a row's end are masked); with conv_a4 = 0 only where the
    channel count is a multiple of 4 and the tensor is 16-byte aligned -- the other shapes then take 4-byte loads"""
    return (Cin % 4 == 0 and aligned) or conv_a4_option != 0


def conv_forward_route(Cin, Cout, k, stride=1, split_option=-1, aligned=True, gemm_wide=1, conv_a4_option=1):
    """(kernel, output-channel tile) of nntk_shim_conv1d at out_mode 0: what nntk_shim_gemm_nt (Cin = K, Cout = N, k = 1) and
    nntk_shim_conv_dx_mfma (Cin = the layer's Cout, Cout = the layer's Cin) run"""
    cout_p = (Cout + 31) & ~31
    assert (CONV_BM - 1) * stride + k <= 192       # the wide-window instantiations are not reached from the training products
    if Cin * k < CONV_VALU_KDIM or Cout < CONV_VALU_COUT:
        return CONV_VALU, None
    a4 = conv_a4(Cin, aligned, conv_a4_option)
    if split_option == 0:
        return CONV_EXACT, 128 if cout_p % 128 == 0 else 64 if cout_p % 64 == 0 else 32
    if k == 1 and cout_p % 256 == 0 and a4 and gemm_wide != 0:
        return CONV_SPLIT, 256
    return CONV_SPLIT, 128 if cout_p % 128 == 0 else 64 if cout_p % 64 == 0 else 32


def pack_sizes(Cin, Cout):
    """nntk_shim_conv_pack_sizes"""
    return (Cin + CONV_KC - 1) & ~(CONV_KC - 1), (Cout + 31) & ~31


# ---- outer_accumulate ---------------------------------------------------------------------------------------------------------------
# name -> (rows, I, K, a_shift_T, the kernel the code's conditions route it to, what it is there for)
OUTER_VALU = {
    "a": (5, 3, 7, 0, VALU, "rows < 32 slices: most slices are empty"),
    "b": (200, 33, 300, 0, VALU, "K > 256: thread k strides"),
    "c": (60, 1, 1, 0, VALU, "smallest I and K"),
    "d": (3 * 7, 5, 9, 7, VALU, "time shift"),
    "e": (6, 4, 8, 1, VALU, "T = 1: A contributes nothing"),
    "f": (4097, 0, 600, 0, COLSUM, "I = 0: the column sums alone, NULL d_A"),
    "g": (31, 40, 40, 0, VALU, "I, K >= 32 below 2^27 MACs; 31 rows: slice 0 is empty, every other holds one row"),
}
OUTER_PLAIN = {
    "one_tile": (131072, 32, 32, 0, PLAIN, "one tile, 32 slices"),
    "ragged": (31291, 33, 130, 0, PLAIN, "odd rows, ragged I and K, second K tile mostly empty"),
    "tiles_2x3": (4019, 130, 257, 0, PLAIN, "2 x 3 tiles, the bias row written once, slice lengths no multiple of 8"),
    "few_slices": (1489, 300, 301, 0, PLAIN, "slices = rows / 64 = 23 < 32"),
    "half_masked": (2731, 96, 512, 0, PLAIN, "I in 65..127: wave pair 1 half masked"),
    "narrow_k": (11187, 300, 40, 0, PLAIN, "K in 33..63: the second wave of every pair leaves, the first is part masked; three I tiles"),
}
OUTER_SHIFT = {
    "T1": (32768, 64, 64, 1, PLAIN_SHIFT, "T = 1: A contributes nothing"),
    "T2": (8195 * 2, 96, 96, 2, PLAIN_SHIFT, "short sequence; slices start at t = 1 too"),
    "T3": (5463 * 3, 96, 96, 3, PLAIN_SHIFT, "odd row total; tt wraps inside a trip"),
    "T7": (2397 * 7, 40, 200, 7, PLAIN_SHIFT, "B odd; slice starts at every phase of t, t = 0 included; T shorter than a trip"),
    "Tlong": (2 * 16400, 64, 64, 16400, PLAIN_SHIFT, "a sequence longer than a slice"),
}
OUTER_MFMA = dict(OUTER_PLAIN, **OUTER_SHIFT)
OUTER_ALL = dict(OUTER_VALU, **OUTER_MFMA)


def _ints(rng, *shape):
    return rng.integers(LO, HI + 1, shape).astype(np.int64)


def shifted(A, T):
    """row (b, t) -> row (b, t - 1), zeros at t = 0"""
    if T <= 0:
        return A
    S = np.zeros_like(A)
    S[1:] = A[:-1]
    S[::T] = 0
    return S


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name))


@functools.lru_cache(maxsize=None)
def outer_case(name):
    """dict(A, B, C0, c0: int64 inputs; C, c: the int64 result of the definition); computed once, shared, never changed"""
    rows, I, K, T, _, _ = OUTER_ALL[name]
    rng = np.random.default_rng(1000 + _seed(name))
    A, B = _ints(rng, rows, I), _ints(rng, rows, K)
    Cs, cs = rng.integers(-C0, C0 + 1, (I, K)).astype(np.int64), rng.integers(-C0, C0 + 1, (K,)).astype(np.int64)
    Cs[Cs == 0] = 7
    cs[cs == 0] = 7
    return dict(A=A, B=B, C0=Cs, c0=cs, C=Cs + shifted(A, T).T @ B, c=cs + B.sum(axis=0))


def exact_cap(terms, initial=0):
    """every partial sum of `terms` products of integers in -3 .. 3 onto |initial| is an integer below 2^24: exact in f32"""
    return 9 * terms + initial < EXACT


# ---- nntk_shim_conv1d_grad ----------------------------------------------------------------------------------------------------------
# name -> (B, T, Cin, Cout, k, stride, Tout, the d_W kernel, what it is there for)
CONV_MFMA = {
    "rps1": (5300, 5, 40, 128, 5, 1, 1, GENERAL, "rps = Tout = 1: both sequence-crossing corrections every row pair"),
    "rps2": (2650, 8, 40, 128, 5, 2, 2, GENERAL, "rps = 2, stride 2, a trailing input row no window reads"),
    "rps3": (1767, 7, 40, 128, 5, 1, 3, GENERAL, "odd rps"),
    "mixed_cout72": (54, 143, 36, 72, 7, 1, 137, GENERAL, "Cout in 65..127; B Tout = 7398, the fewest rows past 2^27"),
    "mixed_cin33": (29, 489, 33, 96, 3, 1, 487, GENERAL, "ragged Cin; B Tout = 14123, the fewest rows past 2^27"),
}
CONV_VALU_CASES = {
    "one_row": (1, 5, 3, 1, 5, 1, 1, CONV_DW_VALU, "one row: 31 empty slices; Cout = 1"),
    "cout300": (2, 9, 2, 300, 2, 1, 8, CONV_DW_VALU, "Cout > 256: thread o strides"),
    "stride_gt_k": (2, 17, 5, 3, 2, 3, 6, CONV_DW_VALU, "stride > k: untouched input rows get exactly 0"),
    "tout0": (3, 4, 2, 4, 5, 1, 0, CONV_DW_VALU, "Tout = 0: d_W, d_b, d_X all zero"),
}
CONV_ALL = dict(CONV_MFMA, **CONV_VALU_CASES)


def conv_route(name):
    B, T, Cin, Cout, k, stride, Tout = CONV_ALL[name][:7]
    rows = B * max(Tout, 0)
    if rows == 0:
        return CONV_DW_VALU, GRAD_SLICES
    kern, slices = outer_route(rows, k * Cin, Cout, 0, rps=Tout, row_pitch=stride * Cin)
    return (CONV_DW_VALU, GRAD_SLICES) if kern == VALU else (kern, slices)


def conv_grad_reference(x, W, dout, stride):
    """Conv1dCalculateGradient's definition on [B][T][Cin], [Cout][Cin][k], [B][Tout][Cout] -> d_W [Cout][Cin][k], d_b, d_X"""
    B, T, Cin = x.shape
    Cout, _, k = W.shape
    Tout = dout.shape[1]
    dW, dX = np.zeros(W.shape, x.dtype), np.zeros(x.shape, x.dtype)
    d2 = dout.reshape(B * Tout, Cout)
    for kk in range(k):
        if Tout > 0:
            win = x[:, kk:kk + (Tout - 1) * stride + 1:stride, :]
            dW[:, :, kk] = d2.T @ win.reshape(B * Tout, Cin)
            dX[:, kk:kk + (Tout - 1) * stride + 1:stride, :] += (d2 @ W[:, :, kk]).reshape(B, Tout, Cin)
    return dW, d2.sum(axis=0), dX


@functools.lru_cache(maxsize=None)
def conv_case(name):
    B, T, Cin, Cout, k, stride, Tout = CONV_ALL[name][:7]
    rng = np.random.default_rng(2000 + _seed(name))
    x, W, dout = _ints(rng, B, T, Cin), _ints(rng, Cout, Cin, k), _ints(rng, B, max(Tout, 0), Cout)
    dW, db, dX = conv_grad_reference(x, W, dout, stride)
    return dict(x=x, W=W, dout=dout, dW=dW, db=db, dX=dX)


# ---- nntk_shim_rows_times_rowmat, nntk_shim_gemm_nt, nntk_shim_conv_dx_mfma, nntk_shim_transpose ------------------------------------
ROWMAT = ((1, 1, 1), (7, 33, 130), (300, 5, 1000))                       # rows, I, K

# M, N, K, (kernel, output-channel tile), what it is there for
GEMM_NT = (
    (129, 32, 16, (CONV_SPLIT, 32), "tile edge in M; the smallest N and K the MFMA kernel takes"),
    (130, 1000, 72, (CONV_SPLIT, 256), "N padded to 1024: the wide tile with 24 masked columns; K % 16 != 0 with the A side unpadded"),
    (130, 96, 72, (CONV_SPLIT, 32), "N_p % 32 tile, three of them; K % 16 != 0"),
    (257, 128, 130, (CONV_SPLIT, 128), "K % 4 != 0: masked 16-byte window loads; with conv_a4 = 0 the 4-byte loads"),
    (200, 192, 64, (CONV_SPLIT, 64), "N_p % 64 tile"),
    (128, 256, 64, (CONV_SPLIT, 256), "the 128 x 256 wide tile"),
    (100, 24, 40, (CONV_VALU, None), "N < 32: conv1d_valu_kernel through the packed layout"),
)
GEMM_NT_OPTION_ROW = 3                               # the row repeated with gemm_split_bf16 = 0 and with conv_a4 = 0


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K):
    rng = np.random.default_rng(3000 + 7 * M + 3 * N + K)
    A, Bw = _ints(rng, M, K), _ints(rng, N, K)
    Cs = rng.integers(-C0, C0 + 1, (M, N)).astype(np.int64)
    Cs[Cs == 0] = 7
    return dict(A=A, Bw=Bw, C0=Cs, P=A @ Bw.T)


# B, Tout, Cin, Cout, k, output-channel tile of the d_X convolution (its Cout is the layer's Cin), what it is there for
CONV_DX = (
    (3, 129, 32, 16, 5, 32, "smallest channels the host gate admits; T = 133 crosses a 128-row tile"),
    (2, 1, 33, 40, 3, 64, "Tout = 1"),
    (2, 200, 40, 128, 1, 64, "k = 1: no padding rows"),
    (1, 130, 64, 24, 9, 64, "larger k"),
)


@functools.lru_cache(maxsize=None)
def conv_dx_case(B, Tout, Cin, Cout, k):
    rng = np.random.default_rng(4000 + 11 * B + 5 * Tout + 3 * Cin + Cout + k)
    W, dout = _ints(rng, Cout, Cin, k), _ints(rng, B, Tout, Cout)
    x = np.zeros((B, Tout + k - 1, Cin), np.int64)
    return dict(W=W, dout=dout, dX=conv_grad_reference(x, W, dout, 1)[2])


TRANSPOSE = ((1, 1, 0), (33, 65, 0), (35, 31, 5), (64, 32, 1))           # R, C, shift_T


# ---- the float cases: one per MFMA form ---------------------------------------------------------------------------------------------
def gamma(n):
    """any summation order of n terms, products fused or rounded: |err| <= gamma_n * sum |terms|"""
    u = 2.0 ** -24
    return n * u / (1.0 - n * u)


def outer_chain(rows, slices):
    """n of the exact-f32 forms: the longest slice's chain, one addition per slice in outer_reduce_kernel, and one"""
    starts = slice_starts(rows, slices)
    return max(b - a for a, b in zip(starts, starts[1:])) + slices + 1


# ---- ctypes -------------------------------------------------------------------------------------------------------------------------
_vp, _l, _i, _sz = C.c_void_p, C.c_long, C.c_int, C.c_size_t
SHIM_SIGNATURES = {
    "nntk_shim_outer_scratch_floats": (_sz, [_i, _i]),
    "nntk_shim_outer_accumulate": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i]),
    "nntk_shim_rows_times_rowmat": (_i, [_vp, _vp, _vp, _l, _i, _i]),
    "nntk_shim_conv1d_grad_scratch_floats": (_sz, [_i, _i, _i]),
    "nntk_shim_conv1d_grad": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i]),
    "nntk_shim_gemm_nt_scratch_floats": (_sz, [_i, _i]),
    "nntk_shim_gemm_nt": (_i, [_vp, _vp, _vp, _vp, _vp, _l, _i, _i, _i]),
    "nntk_shim_transpose": (_i, [_vp, _vp, _l, _i, _i]),
    "nntk_shim_conv_dx_pack_floats": (_sz, [_i, _i, _i]),
    "nntk_shim_conv_dx_mfma": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i]),
}


def declare(lib):
    """argtypes / restype of the shim entry points the tests call with device pointers"""
    for name, (res, args) in SHIM_SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = res, args
    return lib
