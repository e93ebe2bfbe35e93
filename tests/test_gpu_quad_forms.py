"""hhgt_quad_forms (x^T A x of every variant: the f64 MFMA over variant-major planes with the second factor in the epilogue)
against numpy: exact on quarters at every shape at which the kernel takes another path, matrices that catch a wrong
triangle, a wrong factor 2 or a dropped last block, the output's extent, the error bound of include/hhgt.h on real values,
the arguments."""
import numpy as np
import pytest
import torch

from haplohyped_varawareml_amd._lib import HhgtError
from tests.test_gpu_assoc import guarded, unpack
from tests.test_gpu_ld import random_vplanes

pytestmark = pytest.mark.gpu


def np_x(planes, coef):
    """x [n_var, 32 sw] as include/hhgt.h defines it: (c0 HET + c1 COMPLETE) + c2 HOM_ALT of the bits"""
    bits = unpack(planes)
    return coef[:, 0, None] * bits[0] + coef[:, 1, None] * bits[1] + coef[:, 2, None] * bits[2]


def np_quad(planes, coef, A):
    x = np_x(planes, coef)
    return ((x @ A) * x).sum(axis=1)


def dev(ctx, a):
    return torch.from_numpy(np.ascontiguousarray(a.view(np.int32) if a.dtype == np.uint32 else a)).to(ctx.device)


def quarters(rng, shape):
    return rng.integers(-8, 9, shape) / 4.0                            # multiples of 1/4 in [-2, 2]


def symmetric(a):
    return np.triu(a) + np.triu(a, 1).T


N_VARS = (1, 15, 16, 17, 127, 128, 129, 130)       # the 16-variant wave and the 128-variant workgroup, either side


@pytest.mark.parametrize("sw", [1, 3, 4, 5, 8, 9, 79])                 # the 128-row block (4 words) and its ragged last one
def test_kernel_is_exact_on_quarters(ctx, sw):
    """A, the coefficients and so x are multiples of 1/4 in [-2, 2]: every product x a x is a multiple of 1/64 below 8 and
    every partial sum a multiple of 1/64 below 2^53 / 64, so the sum is exact in any order"""
    rng = np.random.default_rng(sw)
    A = symmetric(quarters(rng, (32 * sw, 32 * sw)))
    d_A = dev(ctx, A)
    for n_var in N_VARS:
        planes, _ = random_vplanes(rng, n_var, sw)
        coef = quarters(rng, (n_var, 3))
        want = np_quad(planes, coef, A)
        d_planes, d_coef = dev(ctx, planes), dev(ctx, coef)
        got = ctx.quad_forms(d_planes, d_coef, d_A)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (n_var,)
        assert np.array_equal(got.cpu().numpy(), want), (sw, n_var)
        # into the caller's tensor: every entry overwritten, nothing beside it touched, the same bits again
        buf, view = guarded(ctx, (n_var,))
        assert ctx.quad_forms(d_planes, d_coef, d_A, q=view) is view
        host = buf.cpu().numpy()
        assert np.isnan(host[:1024]).all() and np.isnan(host[-1024:]).all()
        assert np.array_equal(host[1024:-1024].view(np.uint64), got.cpu().numpy().view(np.uint64)), (sw, n_var)


@pytest.mark.parametrize("sw", [5, 9])             # two row blocks with a ragged second, three with a ragged third
def test_kernel_structure(ctx, sw):
    rng = np.random.default_rng(40 + sw)
    n, n_var = 32 * sw, 33
    planes, _ = random_vplanes(rng, n_var, sw)
    coef = quarters(rng, (n_var, 3))
    x = np_x(planes, coef)
    d_planes, d_coef = dev(ctx, planes), dev(ctx, coef)
    run = lambda A: ctx.quad_forms(d_planes, d_coef, dev(ctx, A)).cpu().numpy()
    # a diagonal: the sum of d x^2, every row once
    d = quarters(rng, n)
    assert np.array_equal(run(np.diag(d)), (x * x * d).sum(axis=1))
    # one symmetric pair (s, t): 2 a x(s) x(t) — in one word, in two words of a block, in two blocks, in the last block
    for s, t in ((3, 17), (5, 100), (70, 127), (2, 130), (127, 128), (100, n - 1), (n - 2, n - 1), (129, n - 30)):
        A = np.zeros((n, n))
        A[s, t] = A[t, s] = 0.75
        assert np.array_equal(run(A), 1.5 * x[:, s] * x[:, t]), (s, t)
    # ones: the square of the sum
    assert np.array_equal(run(np.ones((n, n))), x.sum(axis=1) ** 2)
    # only the promised triangle is needed: the blocks of 128 on the diagonal in full, above them the upper triangle
    A = symmetric(quarters(rng, (n, n)))
    upper = A.copy()
    for s in range(n):
        upper[s, :128 * (s // 128)] = 0.0
    assert np.array_equal(run(upper), np_quad(planes, coef, A))


def test_kernel_layout_and_zeros(ctx):
    rng = np.random.default_rng(7)
    sw, n_var = 5, 40
    A = symmetric(quarters(rng, (32 * sw, 32 * sw)))
    d_A = dev(ctx, A)
    coef = quarters(rng, (n_var, 3))
    planes, _ = random_vplanes(rng, n_var, sw)
    zeros = torch.zeros((3, n_var, sw), dtype=torch.int32, device=ctx.device)
    assert not ctx.quad_forms(zeros, dev(ctx, coef), d_A).any()
    assert not ctx.quad_forms(dev(ctx, planes), torch.zeros((n_var, 3), dtype=torch.float64, device=ctx.device), d_A).any()
    # any bits: HET and HOM_ALT need not lie inside COMPLETE, nor apart — the bits define the arithmetic
    anyb = rng.integers(0, 1 << 32, (3, n_var, sw), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(ctx.quad_forms(dev(ctx, anyb), dev(ctx, coef), d_A).cpu().numpy(), np_quad(anyb, coef, A))
    full = np.full((3, n_var, sw), 0xffffffff, dtype=np.uint32)
    assert np.array_equal(ctx.quad_forms(dev(ctx, full), dev(ctx, coef), d_A).cpu().numpy(), coef.sum(axis=1) ** 2 * A.sum())


@pytest.mark.parametrize("n_var, sw", [(130, 79), (65, 8), (17, 3)])
def test_kernel_error_bound_on_real_values(ctx, n_var, sw):
    """within 32 sw 2^-51 |x|^T |A| |x| of numpy's float64: hhgt_quad_forms' first-order bound (2 n + 2) 2^-53 |x|^T |A| |x|,
    n = 32 sw, doubled for the second-order terms and for numpy's own summation (x itself is the same bits on both sides)"""
    rng = np.random.default_rng(n_var)
    A = rng.normal(size=(32 * sw, 32 * sw))
    A = (A + A.T) / 2.0
    coef = rng.normal(size=(n_var, 3))
    planes, _ = random_vplanes(rng, n_var, sw)
    x = np_x(planes, coef)
    want = ((x @ A) * x).sum(axis=1)
    bound = 32 * sw * 2.0 ** -51 * ((np.abs(x) @ np.abs(A)) * np.abs(x)).sum(axis=1)
    got = ctx.quad_forms(dev(ctx, planes), dev(ctx, coef), dev(ctx, A))
    again = ctx.quad_forms(dev(ctx, planes), dev(ctx, coef), dev(ctx, A))
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))                  # deterministic
    err = np.abs(got.cpu().numpy() - want)
    print(f"quad_forms {n_var} x {32 * sw}: largest error / bound = {(err / np.maximum(bound, 1e-300)).max():.3g}")
    assert (err <= bound).all()


def test_kernel_arguments(ctx):
    d = ctx.device
    f64 = lambda *shape: torch.ones(shape, dtype=torch.float64, device=d)
    planes = torch.zeros((3, 5, 2), dtype=torch.int32, device=d)
    coef, A = f64(5, 3), f64(64, 64)
    assert tuple(ctx.quad_forms(planes, coef, A).shape) == (5,)
    for kw in (dict(coef=coef.float()), dict(coef=coef[:4]), dict(coef=f64(5, 4)), dict(coef=coef.cpu()),
               dict(coef=f64(5, 6)[:, ::2]), dict(coef=coef[:, 0]),
               dict(a=A.float()), dict(a=A[:63]), dict(a=f64(96, 96)), dict(a=A.cpu()), dict(a=f64(64, 128)[:, ::2]), dict(a=A[0]),
               dict(vplanes=planes.float()), dict(vplanes=planes[:2]), dict(vplanes=planes[:, :, :1]), dict(vplanes=planes[:, ::2]),
               dict(q=torch.zeros(5, dtype=torch.float32, device=d)), dict(q=f64(6)), dict(q=f64(10)[::2]), dict(q=f64(5, 1))):
        with pytest.raises(ValueError):
            ctx.quad_forms(**{**dict(vplanes=planes, coef=coef, a=A), **kw})
    # rows of more than 1024 words: the library's refusal, before anything is launched (the matrix is allocated, never touched)
    wide = torch.zeros((3, 1, 1025), dtype=torch.int32, device=d)
    with pytest.raises(HhgtError, match="words"):
        ctx.quad_forms(wide, f64(1, 3), torch.empty((32 * 1025, 32 * 1025), dtype=torch.float64, device=d))
    # no variant: an empty result; no sample word: zeros
    assert tuple(ctx.quad_forms(planes[:, :0].contiguous(), coef[:0], A).shape) == (0,)
    none = ctx.quad_forms(torch.zeros((3, 5, 0), dtype=torch.int32, device=d), coef, f64(0, 0),
                          q=torch.full((5,), float("nan"), dtype=torch.float64, device=d))
    assert tuple(none.shape) == (5,) and not none.any()
