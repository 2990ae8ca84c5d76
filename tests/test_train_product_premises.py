"""The premises of the direct tests of the training products (tests/test_gpu_train_products.py), checked without a device: the routing
constants mirrored in tests/train_product_cases.py still stand in the sources, every case is routed to the kernel it is there for, has
the number of slices and the slice boundaries it claims, and satisfies the exactness cap 9 * terms + |initial C| < 2^24 that makes the
integer comparison independent of the summation order.  A moved threshold or a changed slice formula turns red here.  No GPU."""
import os
import re

import numpy as np
import pytest

import train_product_cases as K

HIP = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nntoolkitcore_amd", "csrc")


def _src(*path):
    with open(os.path.join(HIP, *path)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^#define\s+%s\s+(\d+)\s*$" % name, text, re.M)
    assert m, name
    return int(m.group(1))


def _body(text, signature):
    """the text from `signature` up to the next line that closes a function at column 0"""
    at = text.index(signature)
    return text[at:text.index("\n}\n", at)]


def test_mirrored_constants_have_not_drifted():
    train, grad, conv, kern = _src("hip", "train.hip"), _src("hip", "conv1d_grad.hip"), _src("hip", "conv1d.hip"), _src("hip", "conv1d_kernels.hpp")
    assert _define(train, "OUTER_TILE") == K.OUTER_TILE
    assert _define(train, "OUTER_SLICES") == K.OUTER_SLICES
    assert _define(train, "COLMAT_CHUNKS") == K.COLMAT_CHUNKS
    assert _define(grad, "GRAD_SLICES") == K.GRAD_SLICES
    assert _define(kern, "CONV_BM") == K.CONV_BM and _define(kern, "CONV_KC") == K.CONV_KC

    launch = _body(train, "int nntk_outer_mfma_launch(")
    m = re.search(r"if \(!\(I >= (\d+) && K >= (\d+) && rps >= 1 && \(double\)rows \* I \* K >= \(double\)\(1 << (\d+)\)\)\) return 0;", launch)
    assert m and (int(m.group(1)), int(m.group(2)), 1 << int(m.group(3))) == (K.OUTER_MIN_I, K.OUTER_MIN_K, K.MFMA_MACS)
    # the slice formula
    assert "const int ti = (I + OUTER_TILE - 1) / OUTER_TILE, tk = (K + OUTER_TILE - 1) / OUTER_TILE;" in launch
    m = re.search(r"int slices = \((\d+) \+ ti \* tk - 1\) / \(ti \* tk\);", launch)
    assert m and int(m.group(1)) == K.OUTER_WORKGROUPS
    assert "if (slices > OUTER_SLICES) slices = OUTER_SLICES;" in launch
    m = re.search(r"if \(\(long\)slices > rows / (\d+)\) slices = \(int\)\(rows / (\d+)\);", launch)
    assert m and int(m.group(1)) == int(m.group(2)) == K.OUTER_SLICE_MIN_ROWS
    assert "if (slices < 1) slices = 1;" in launch
    # the plain predicate, and which kernel each side of it launches
    m = re.search(r"const bool plain = rps >= rows && row_pitch == I && \(double\)\(rows / slices \+ 2\) \* \(I > K \? I : K\) \* 4 < ([0-9.e]+) && "
                  r"nntk_options\(\)\.train_outer_plain != 0;", launch)
    assert m and float(m.group(1)) == K.PLAIN_BYTES
    order = [launch.index(s) for s in ("if (plain && a_shift_T > 0)", "outer_mfma_plain_kernel<true>", "else if (plain)",
                                       "outer_mfma_plain_kernel<false>", "else\n", "outer_mfma_kernel,")]
    assert order == sorted(order)
    # every sliced kernel cuts its rows the same way
    for name in ("outer_partial_kernel", "colsum_partial_kernel"):
        assert "r0 = rows * blockIdx.y / gridDim.y, r1 = rows * (blockIdx.y + 1) / gridDim.y;" in _body(train, "void %s(" % name)
    for name in ("void outer_mfma_kernel(", "void outer_mfma_plain_kernel("):
        assert "r0 = rows * blockIdx.z / gridDim.z, r1 = rows * (blockIdx.z + 1) / gridDim.z;" in _body(train, name)
        assert "rb += %d)" % K.OUTER_TRIP_ROWS in _body(train, name)
    assert "r0 = rows * blockIdx.y / gridDim.y, r1 = rows * (blockIdx.y + 1) / gridDim.y;" in _body(grad, "void conv1d_dw_partial_kernel(")

    # nntk_shim_outer_accumulate: the MFMA form first, the column sums at I == 0, else the VALU dots on OUTER_SLICES slices
    acc = _body(train, 'extern "C" int nntk_shim_outer_accumulate(')
    assert "I > 0 ? nntk_outer_mfma_launch(d_A, d_B, d_scratch, rows, I, K, a_shift_T, rows, 0, I) : 0" in acc
    assert re.search(r"else if \(I == 0\)\s+hipLaunchKernelGGL\(colsum_partial_kernel, dim3\(\(unsigned\)\(\(K \+ 255\) / 256\), OUTER_SLICES\)", acc)
    assert "hipLaunchKernelGGL(outer_partial_kernel, dim3((unsigned)(I + 1), OUTER_SLICES)" in acc
    assert "return (size_t)OUTER_SLICES * (I + 1) * K;" in train
    # nntk_shim_conv1d_grad: the im2col view it hands over, GRAD_SLICES otherwise
    cg = _body(grad, 'extern "C" int nntk_shim_conv1d_grad(')
    assert "nntk_outer_mfma_launch(d_in, d_dout, d_scratch, rows, ncol, Cout, 0, Tout, (long)T * Cin, (long)stride * Cin)" in cg
    assert "hipLaunchKernelGGL(conv1d_dw_partial_kernel, dim3((unsigned)(k * Cin), GRAD_SLICES)" in cg
    assert "return (size_t)GRAD_SLICES * ((size_t)k * Cin + 1) * Cout;" in grad

    host = _src("host", "train.c")
    m = re.search(r"#define NNTK_TRAIN_MFMA_MACS \(\(double\)\(1 << (\d+)\)\)", host)
    assert m and 1 << int(m.group(1)) == K.MFMA_MACS
    m = re.search(r"const int mfma = \(double\)rows \* I \* K >= NNTK_TRAIN_MFMA_MACS && K >= (\d+) && I >= (\d+);", host)
    assert m and (int(m.group(1)), int(m.group(2))) == (K.GEMM_MIN_K, K.GEMM_MIN_I)
    m = re.search(r"\(double\)rows \* Cout \* k \* Cin >= \(double\)\(1 << (\d+)\) && Cin >= (\d+) && Cout >= (\d+)\)", _src("host", "conv_1d.c"))
    assert m and (1 << int(m.group(1)), int(m.group(2)), int(m.group(3))) == (K.MFMA_MACS, K.DX_MIN_CIN, K.DX_MIN_COUT)

    # the forward kernel's routing, as nntk_shim_gemm_nt and nntk_shim_conv_dx_mfma reach it
    m = re.search(r"if \(!window_fits \|\| Kdim < (\d+) \|\| Cout < (\d+)\) \{", conv)
    assert m and (int(m.group(1)), int(m.group(2))) == (K.CONV_VALU_KDIM, K.CONV_VALU_COUT)
    assert "*Cin_p = (Cin + CONV_KC - 1) & ~(CONV_KC - 1);" in conv and "*Cout_p = (Cout + 31) & ~31;" in conv
    assert "const bool a4 = ((Cin % 4 == 0) && ((size_t)d_in % 16 == 0)) || opt.conv_a4 != 0;" in conv
    assert "if (k == 1 && p.Cout_p % 256 == 0 && a4 && p.quad && opt.gemm_wide != 0) return launch_mfma<2, 2, 2, 4, true, true>(p);" in conv
    common = _src("hip", "nntk_common.hpp")
    assert re.search(r"int conv_a4 = 1;", common) and re.search(r"int gemm_wide = -1;", common) and re.search(r"int gemm_split_bf16 = -1;", common)
    assert re.search(r"int train_outer_plain = -1;", common)
    assert "nntk_shim_conv1d(d_A, d_pack, nullptr, nullptr, 0.f, NNTK_ACT_IDENTITY, 1.f, out, 1, (int)M, K, N, 1, 1, (int)M, 0)" in train
    assert "nntk_shim_conv1d(d_pad, d_wpack, nullptr, nullptr, 0.f, NNTK_ACT_IDENTITY, 1.f, d_dX, B, Tp, Cout, Cin, k, 1, T, 0)" in train


@pytest.mark.parametrize("name", sorted(K.OUTER_ALL))
def test_outer_case_route_slices_and_cap(name):
    rows, I, Kk, T, want, _ = K.OUTER_ALL[name]
    kern, slices = K.outer_route(rows, I, Kk, T)
    assert kern == want, (name, kern)
    assert K.exact_cap(rows, K.C0), name
    macs = rows * I * Kk
    starts = K.slice_starts(rows, slices)
    lengths = [b - a for a, b in zip(starts, starts[1:])]
    if name in K.OUTER_VALU:
        assert macs < K.MFMA_MACS and slices == K.OUTER_SLICES
    else:
        assert macs >= K.MFMA_MACS and I >= K.OUTER_MIN_I and Kk >= K.OUTER_MIN_K
        # ... and the same shape on the general kernel once the option is cleared, on the same slices
        assert K.outer_route(rows, I, Kk, T, plain_option=0) == (K.GENERAL, slices)
    if name == "a":
        assert rows < K.OUTER_SLICES and lengths.count(0) == K.OUTER_SLICES - rows          # empty VALU slices
    if name == "g":
        assert I >= K.OUTER_MIN_I and Kk >= K.OUTER_MIN_K and lengths[0] == 0                # below 2^27 only
    if name == "b":
        assert Kk > 256
    if name == "d":
        assert T > 1 and rows % T == 0 and rows // T > 1
    if name == "e":
        assert T == 1
    if name == "f":
        assert I == 0 and kern == K.COLSUM and Kk > 2 * 256                                   # three workgroups of columns, the last partial
    if name == "one_tile":
        assert slices == 32 and I <= K.OUTER_TILE and Kk <= K.OUTER_TILE and macs == K.MFMA_MACS
    if name == "ragged":
        assert rows % 2 == 1 and slices == 32 and I % 32 and Kk % 64 and Kk - K.OUTER_TILE < 32
        assert any(s % 2 for s in starts[1:-1])
    if name == "tiles_2x3":
        assert (-(-I // K.OUTER_TILE), -(-Kk // K.OUTER_TILE)) == (2, 3) and slices == 32
        assert all(n % K.OUTER_TRIP_ROWS for n in lengths) and any(s % 2 for s in starts[1:-1])
    if name == "few_slices":
        assert slices == rows // K.OUTER_SLICE_MIN_ROWS == 23 < K.OUTER_SLICES
        assert any(n % K.OUTER_TRIP_ROWS for n in lengths) and any(s % 2 for s in starts[1:-1])
    if name == "half_masked":
        assert 64 < I < 128 and I % 32 == 0 and slices == 32
    if name == "narrow_k":
        assert 32 < Kk < 64 and -(-I // K.OUTER_TILE) == 3 and rows % 2 == 1 and slices == 32
    if name in K.OUTER_SHIFT:
        assert T > 0 and rows % T == 0 and slices == 32
        phases = {s % T for s in starts[:-1]}
        if name == "T1":
            assert T == 1
        if name == "T2":
            assert phases == {0, 1}                                                           # slices start at t = 0 and at t = 1
        if name == "T3":
            assert rows % 2 == 1 and phases == {0, 1, 2} and T < K.OUTER_TRIP_ROWS
        if name == "T7":
            assert (rows // T) % 2 == 1 and phases == set(range(7)) and T < K.OUTER_TRIP_ROWS and any(s % 2 for s in starts)
        if name == "Tlong":
            assert T > max(lengths) and rows // T == 2 and T in starts          # the second sequence's t = 0 opens a slice


@pytest.mark.parametrize("name", sorted(K.CONV_ALL))
def test_conv_grad_case_route_slices_and_cap(name):
    B, T, Cin, Cout, k, stride, Tout, want, _ = K.CONV_ALL[name]
    assert Tout == max((T - k) // stride + 1, 0) if T >= k else Tout == 0
    kern, slices = K.conv_route(name)
    assert kern == want, (name, kern)
    rows, ncol = B * Tout, k * Cin
    assert K.exact_cap(max(rows, k * Cout)), name                 # d_W / d_b sum over the rows, d_X over k * Cout
    starts = K.slice_starts(rows, slices)
    if name in K.CONV_MFMA:
        assert rows * ncol * Cout >= K.MFMA_MACS and slices == 32
        assert any(s % Tout for s in starts[:-1]) or Tout == 1    # a slice starts inside a sequence
        assert any(s % 2 for s in starts[:-1])
    else:
        assert rows * ncol * Cout < K.MFMA_MACS and slices == K.GRAD_SLICES
    if name.startswith("rps"):
        assert Tout == int(name[3:]) and ncol == 200 and Cout == 128
    if name == "rps2":
        assert stride == 2 and T > (Tout - 1) * stride + k        # a trailing row outside every window
    if name == "mixed_cout72":
        assert 64 < Cout < 128 and (rows - 1) * ncol * Cout < K.MFMA_MACS      # one row fewer stays on the VALU form
    if name == "mixed_cin33":
        assert Cin % 4 and (rows - 1) * ncol * Cout < K.MFMA_MACS
    if name == "one_row":
        assert rows == 1 < K.GRAD_SLICES and Cout == 1           # empty VALU slices
    if name == "cout300":
        assert Cout > 256
    if name == "stride_gt_k":
        assert stride > k
        dX = K.conv_case(name)["dX"]
        touched = sorted({x * stride + kk for x in range(Tout) for kk in range(k)})
        assert len(touched) < T and not dX[:, [t for t in range(T) if t not in touched], :].any() and dX.any()
    if name == "tout0":
        c = K.conv_case(name)
        assert Tout == 0 and T < k and not c["dW"].any() and not c["db"].any() and not c["dX"].any()


def test_rowmat_gemm_dx_transpose_routes_and_cap():
    for rows, I, Kk in K.ROWMAT:
        assert K.exact_cap(Kk)
    seen = set()
    for M, N, Kk, want, _ in K.GEMM_NT:
        assert K.conv_forward_route(Kk, N, 1) == want, (M, N, Kk)
        assert K.exact_cap(Kk, K.C0)
        seen.add(want)
    assert {t for _, t in seen} == {32, 64, 128, 256, None}       # every tile of the split kernel and the VALU kernel
    M, N, Kk = K.GEMM_NT[K.GEMM_NT_OPTION_ROW][:3]
    assert K.conv_forward_route(Kk, N, 1, split_option=0)[0] == K.CONV_EXACT
    assert Kk % 4 and K.conv_a4(Kk) and not K.conv_a4(Kk, conv_a4_option=0)
    assert any(M % K.CONV_BM == 1 for M, *_ in K.GEMM_NT) and any(Kk % K.CONV_KC for _, _, Kk, *_ in K.GEMM_NT)
    assert K.pack_sizes(72, 1000) == (80, 1024)                   # 1000 columns pad to 1024: the wide tile, not the 32-wide one
    for B, Tout, Cin, Cout, k, tile, _ in K.CONV_DX:
        assert Cin >= K.DX_MIN_CIN and Cout >= K.DX_MIN_COUT      # the channels the host gate admits
        assert K.conv_forward_route(Cout, Cin, k) == (K.CONV_SPLIT, tile)
        assert K.exact_cap(k * Cout)
    assert K.CONV_DX[0][2:4] == (K.DX_MIN_CIN, K.DX_MIN_COUT) and K.CONV_DX[0][1] + K.CONV_DX[0][4] - 1 > K.CONV_BM
    assert any(s > 0 for _, _, s in K.TRANSPOSE) and any(s == 1 for _, _, s in K.TRANSPOSE)


def test_never_reached_routes_are_each_hit():
    """the routes no other test reaches, and the case of this suite that does"""
    assert any(K.outer_route(r, I, Kk, T, plain_option=0)[0] == K.GENERAL and T > 0 for r, I, Kk, T, *_ in K.OUTER_SHIFT.values())
    assert {K.CONV_ALL[n][6] for n in K.CONV_MFMA if K.conv_route(n)[0] == K.GENERAL} >= {1, 2, 3}
    assert len(K.GEMM_NT) > 0                                     # every row runs with accumulate 0 and 1
    assert any(s > 0 for _, _, s in K.TRANSPOSE)
    assert any(K.outer_route(r, I, Kk, T)[0] == K.COLSUM for r, I, Kk, T, *_ in K.OUTER_VALU.values())
    assert any(r < K.OUTER_SLICES for r, *_ in K.OUTER_VALU.values())
    assert any(c[0] * c[6] < K.GRAD_SLICES and c[6] > 0 for c in K.CONV_VALU_CASES.values())
    assert any(c[6] == 0 for c in K.CONV_VALU_CASES.values())


def test_float_bound_is_small_against_a_dropped_row():
    """gamma_n of the longest chain here stays far below one term's weight: a row left out or counted twice cannot hide in it"""
    n = max(K.outer_chain(rows, K.outer_slices(rows, I, Kk)) for rows, I, Kk, *_ in K.OUTER_MFMA.values())
    assert n < 4200 and K.gamma(n) < 2.6e-4
    assert np.isclose(K.gamma(1), 2.0 ** -24)
