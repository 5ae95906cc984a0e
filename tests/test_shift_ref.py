"""The host restatement of multi-shift CG (tests/shift_ref.py) against what it restates: an independent CG solve of every shifted
system.  No GPU.

Systems: the 33 x 29 five-point Laplacian in float64 with shifts {0.05, 0.7, 6}, and L - (0.3 + 0.2i) I in complex128 (complex
symmetric, unconjugated dots) with shifts {0.05 + 0.1i, 0.7 - 0.3i, 6 + i}; 30 iterations.  In exact arithmetic x_j of the shifted
recurrence IS the CG iterate of A + sigma_j I, so the two differ by rounding alone: the bound is 1e-11 relative (measured: at most
1.4e-15 real, 2.8e-14 complex).  The long run shows what the ratio form is for: on the 200 x 200 Laplacian with sigma = 6, zeta is
exactly 0.0 after 900 iterations and x_j stays finite with a true residual at rounding level."""
import numpy as np
import scipy.sparse as sp

import shift_ref as M

NX, NY, ITERS = 33, 29, 30
CASES = {"f64": (np.float64, (0.05, 0.7, 6.0)), "c128": (np.complex128, (0.05 + 0.1j, 0.7 - 0.3j, 6 + 1j))}


def _system(name):
    dtype, sig = CASES[name]
    n = NX * NY
    rng = np.random.default_rng(5)
    if name == "c128":
        return M.shifted_laplace2d(NX, NY, 0.3 + 0.2j), (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(dtype), sig
    return M.laplace2d(NX, NY), rng.standard_normal(n).astype(dtype), sig


def test_shifted_iterates_are_the_iterates_of_the_shifted_systems():
    for name in CASES:
        A, b, sig = _system(name)
        n = b.size
        got = M.mscg(A, b, sig, ITERS)
        xs0, h0 = M.cg(A.astype(b.dtype), b, ITERS)
        assert np.array_equal(got["x"], xs0) and np.array_equal(got["history"], h0)       # the seed is the plain recurrence
        assert np.all(got["zeta"][0] == 1) and got["zeta"].shape == (ITERS + 1, len(sig))
        for j, s in enumerate(sig):
            xi, hi = M.cg((A + s * sp.eye(n)).tocsr().astype(b.dtype), b, ITERS)
            err = np.linalg.norm(got["xs"][j] - xi) / np.linalg.norm(xi)
            # the residual of the shifted system is zeta r: its r.r is zeta^2 times the seed's
            herr = np.max(np.abs(got["zeta"][:, j] ** 2 * got["history"] - hi) / np.abs(hi))
            print(f"  {name} sigma {s}: x_j against separate CG {err:.2e} (< 1e-11), delta_k^j against its history {herr:.2e}, |zeta_30| "
                  f"{abs(got['zeta'][-1, j]):.3e}")
            assert err < 1e-11
            assert herr < 1e-9


def test_zero_shift_is_the_seed():
    A, b, _ = _system("f64")
    got = M.mscg(A, b, [0.0], ITERS)
    assert np.array_equal(got["xs"][0], got["x"]) and np.all(got["zeta"] == 1) and np.all(got["theta"] == 1)


def test_zeta_underflows_to_zero_and_nothing_breaks():
    A = M.laplace2d(200, 200)
    b = np.random.default_rng(3).standard_normal(200 * 200)
    got = M.mscg(A, b, [6.0, 0.01], 900)
    assert got["zeta"][-1, 0] == 0.0 and got["zeta"][-1, 1] != 0.0
    assert np.isfinite(got["xs"]).all() and np.isfinite(got["x"]).all()
    res = [np.linalg.norm(b - (A + s * sp.eye(b.size)) @ x) / np.linalg.norm(b) for s, x in zip((6.0, 0.01), got["xs"])]
    print(f"  true residuals after 900 iterations: sigma 6 {res[0]:.2e}, sigma 0.01 {res[1]:.2e}")
    assert res[0] < 1e-12 and res[1] < 1e-6


def test_update_bits_is_the_plain_expression_on_the_real_types():
    """numpy arithmetic on a real type rounds once per operation, so the type-true form must equal it bit for bit; for the complex
    types it is the component form of the kernel (numpy may fuse a complex product)"""
    rng = np.random.default_rng(1)
    for dtype in (np.float32, np.float64):
        r = rng.standard_normal((2, 37)).astype(dtype)
        xs, ds = (rng.standard_normal((3, 2, 37)).astype(dtype) for _ in range(2))
        al, be, ze = (rng.standard_normal((3, 2)).astype(dtype) for _ in range(3))
        nx, nd = M.update_bits(r, xs, ds, al, be, ze)
        assert np.array_equal(nx, xs + al[:, :, None] * ds)
        assert np.array_equal(nd, ze[:, :, None] * r[None] + be[:, :, None] * ds)
    for dtype in (np.complex64, np.complex128):
        r = (rng.standard_normal((1, 5)) + 1j * rng.standard_normal((1, 5))).astype(dtype)
        xs, ds = ((rng.standard_normal((2, 1, 5)) + 1j * rng.standard_normal((2, 1, 5))).astype(dtype) for _ in range(2))
        al, be, ze = ((rng.standard_normal((2, 1)) + 1j * rng.standard_normal((2, 1))).astype(dtype) for _ in range(3))
        nx, nd = M.update_bits(r, xs, ds, al, be, ze)
        eps = np.finfo(dtype).eps
        assert np.allclose(nx, xs + al[:, :, None] * ds, rtol=0, atol=16 * eps * 10)
        assert np.allclose(nd, ze[:, :, None] * r[None] + be[:, :, None] * ds, rtol=0, atol=16 * eps * 10)
