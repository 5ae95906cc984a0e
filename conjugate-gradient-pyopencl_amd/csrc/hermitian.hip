// Vector and scalar steps of CGAMD_HERMITIAN handles: CG for a complex Hermitian positive-definite matrix, with the conjugated inner
// product <a, b> = sum conj(a_i) b_i where every other loop of the library takes the reference's unconjugated a.b (COCG, right for
// its complex-symmetric Helmholtz matrices, not a CG recurrence for A = A^H).  Complex value types only: on the real ones the two
// products coincide and the handle runs the loops it always ran.
//
// The iteration is four launches:
//   SpMV                 q = A d with the fused dot taken against dc = conj(d): every SpMV kernel reads the vector of its dot
//                        (dvec) apart from the one it gathers, so d^H q comes out of all of them unchanged
//   herm_alpha           alpha = rho / Re(d^H q), the partials summed in a fixed order
//   herm_axpy_dot        r -= alpha q, partials of r^H r (with a diagonal M also of r^H (m .* r))
//   herm_aypx_beta_x     beta = rho' / rho, delta, history and the stop decision in the prologue; x += alpha d,
//                        d = beta d + r (d = beta d + m .* r), dc = conj(d)
// rho is r^H r, or Re(r^H z) with z = m .* r; alpha and beta are REAL and stored in the value type with an imaginary part of +0,
// like delta and the history, which holds r^H r in both cases.  Products are formed in the value type as vmul(vconj(a), b) and
// summed in the accumulator type, as the unconjugated dots are (vector.hip): Im(conj(a) a) = a.x a.y + (-a.y) a.x is exactly +0.
//
// Layout and reductions as in vector.hip: work-groups of 256 threads on the handle's vector grid, grid.y = right-hand side, 16-byte
// packs with a scalar tail, block_sum and then a fixed-order pass over the per-work-group partials; no atomics on data.  GUARD is the
// instantiation cgamd_solver_iterate_until launches (stop_device.h): the alpha step and the r update leave on stop[], the d step on
// live[].
#include "cgamd_internal.h"
#include "device_types.h"
#include "device_mem.h"
#include "reduce_device.h"
#include "stop_device.h"
#include "launch_util.h"

namespace cgamd {

// a real scalar in the complex value type: imaginary part +0
template <typename T> CG_DEV T herm_real(double re) {
    T v = vzero<T>();
    v.x = (typename VT<T>::real)re;
    return v;
}
// a / b of two real scalars kept in the value type, rounded like the other loops' alpha and beta: in the accumulator type, then once
template <typename T> CG_DEV T herm_ratio(T a, T b) { return herm_real<T>((double)a.x / (double)b.x); }

// set_rhs: d = r (PRE: d = m .* r), dc = conj(d); partials of r^H r (PRE: and of r^H d)
template <typename T, int BLOCK, bool VEC, bool PRE>
__global__ __launch_bounds__(BLOCK) void herm_init_kernel(int n, const T *__restrict__ rv, T *__restrict__ d, T *__restrict__ dc,
                                                          const T *__restrict__ m, long long mp, long long ld,
                                                          typename VT<T>::acc *__restrict__ part_rz,
                                                          typename VT<T>::acc *__restrict__ part_rr) {
    using A = typename VT<T>::acc;
    __shared__ A red[BLOCK / kWave];
    const int r = blockIdx.y;
    rv += (long long)r * ld; d += (long long)r * ld; dc += (long long)r * ld;
    if (PRE) m += (long long)r * mp;
    A arz = vzero<A>(), arr = vzero<A>();
    constexpr int E = Pack<T>::N;
    const long long stride = (long long)gridDim.x * BLOCK;
    long long i0 = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (VEC) {
        const long long npack = n / E;
        for (long long i = i0; i < npack; i += stride) {
            const Pack<T> pr = ld_pack(rv + i * E);
            Pack<T> pd = pr, pc;
            if (PRE) {
                const Pack<T> pm = ld_pack(m + i * E);
#pragma unroll
                for (int k = 0; k < E; ++k) pd.v[k] = vmul(pm.v[k], pr.v[k]);
            }
#pragma unroll
            for (int k = 0; k < E; ++k) {
                const T rc = vconj(pr.v[k]);
                pc.v[k] = vconj(pd.v[k]);
                if (PRE) arz = vadd(arz, to_acc(vmul(rc, pd.v[k])));
                arr = vadd(arr, to_acc(vmul(rc, pr.v[k])));
            }
            st_pack(d + i * E, pd);
            st_pack(dc + i * E, pc);
        }
        i0 += npack * E;
    }
    for (long long i = i0; i < n; i += stride) {
        const T rn = rv[i], rc = vconj(rn);
        const T dn = PRE ? vmul(m[i], rn) : rn;
        d[i] = dn;
        dc[i] = vconj(dn);
        if (PRE) arz = vadd(arz, to_acc(vmul(rc, dn)));
        arr = vadd(arr, to_acc(vmul(rc, rn)));
    }
    if (PRE) {
        const A trz = block_sum<BLOCK>(arz, red);
        if (threadIdx.x == 0) part_rz[(long long)r * gridDim.x + blockIdx.x] = trz;
    }
    const A trr = block_sum<BLOCK>(arr, red);
    if (threadIdx.x == 0) part_rr[(long long)r * gridDim.x + blockIdx.x] = trr;
}

// set_rhs: delta = rho0 (r^H r, PRE: Re(r^H z), also into rho2[0]), history[0] = r^H r, iter = 0
template <typename T, bool PRE>
__global__ __launch_bounds__(kScalarBlock) void herm_delta0_kernel(const typename VT<T>::acc *part_rz, const typename VT<T>::acc *part_rr,
                                                                   int P, int nrhs, T *delta, T *history, T *rho2, int *iter) {
    __shared__ typename VT<T>::acc smem[kScalarBlock / kWave];
    const int r = blockIdx.x;
    const auto rr = sum_partials_block(part_rr + (long long)r * P, P, smem);
    double rho = rr.x;
    if (PRE) {
        __syncthreads();
        rho = sum_partials_block(part_rz + (long long)r * P, P, smem).x;
    }
    if (threadIdx.x == 0) {
        delta[r] = herm_real<T>(rho);
        if (PRE) rho2[r] = herm_real<T>(rho);
        history[r] = herm_real<T>(rr.x);
        if (r == 0) *iter = 0;
    }
}

// alpha[r] = delta[r] / Re(d^H q)[r]; block 0 advances the iteration counter, which only later launches read (cg_alpha_kernel)
template <typename T, bool GUARD>
__global__ __launch_bounds__(kScalarBlock) void herm_alpha_kernel(const typename VT<T>::acc *partials, int grid, int K, int nrhs,
                                                                  const T *delta, T *alpha, int *iter, CgStop g) {
    __shared__ typename VT<T>::acc smem[kScalarBlock / kWave];
    const int r = blockIdx.x;
    if (GUARD) {        // the counter moves while anything iterates; a frozen right-hand side retires and leaves
        if (threadIdx.x == 0 && r == 0) stop_advance(g, iter);
        if (g.stop[r] != 0) {
            if (threadIdx.x == 0) stop_retire(g, r);
            return;
        }
    }
    const auto dq = sum_partials_block(partials + (long long)r * grid, grid, smem, K);
    if (threadIdx.x == 0) {
        alpha[r] = herm_ratio(delta[r], from_acc<T>(dq));      // d^H q rounded to the value type before the division, like d.q
        if (!GUARD && r == 0) *iter = *iter + 1;
    }
}

// r -= alpha q ; partials of r^H r (PRE: and of r^H (m .* r))
template <typename T, int BLOCK, bool VEC, bool PRE, bool GUARD>
__global__ __launch_bounds__(BLOCK) void herm_axpy_dot_kernel(int n, const T *__restrict__ q, T *__restrict__ rv, const T *__restrict__ m,
                                                              long long mp, long long ld, const T *__restrict__ alpha,
                                                              typename VT<T>::acc *__restrict__ part_rz,
                                                              typename VT<T>::acc *__restrict__ part_rr, CgStop g) {
    using A = typename VT<T>::acc;
    __shared__ A red[BLOCK / kWave];
    const int r = blockIdx.y;
    if (GUARD && g.stop[r] != 0) return;
    q += (long long)r * ld; rv += (long long)r * ld;
    if (PRE) m += (long long)r * mp;
    const T al = alpha[r];
    A arz = vzero<A>(), arr = vzero<A>();
    constexpr int E = Pack<T>::N;
    const long long stride = (long long)gridDim.x * BLOCK;
    long long i0 = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (VEC) {
        const long long npack = n / E;
        for (long long i = i0; i < npack; i += stride) {
            const Pack<T> pq = ld_pack(q + i * E);
            Pack<T> pr = ld_pack(rv + i * E), pm;
            if (PRE) pm = ld_pack(m + i * E);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                pr.v[k] = vsub(pr.v[k], vmul(al, pq.v[k]));
                const T rc = vconj(pr.v[k]);
                if (PRE) arz = vadd(arz, to_acc(vmul(rc, vmul(pm.v[k], pr.v[k]))));
                arr = vadd(arr, to_acc(vmul(rc, pr.v[k])));
            }
            st_pack(rv + i * E, pr);
        }
        i0 += npack * E;
    }
    for (long long i = i0; i < n; i += stride) {
        const T rn = vsub(rv[i], vmul(al, q[i])), rc = vconj(rn);
        rv[i] = rn;
        if (PRE) arz = vadd(arz, to_acc(vmul(rc, vmul(m[i], rn))));
        arr = vadd(arr, to_acc(vmul(rc, rn)));
    }
    if (PRE) {
        const A trz = block_sum<BLOCK>(arz, red);
        if (threadIdx.x == 0) part_rz[(long long)r * gridDim.x + blockIdx.x] = trz;
    }
    const A trr = block_sum<BLOCK>(arr, red);
    if (threadIdx.x == 0) part_rr[(long long)r * gridDim.x + blockIdx.x] = trr;
}

// beta in the prologue -- every work-group adds the P partials in the same fixed order and holds the same bits, work-group 0
// records beta, delta, history[iter] (r^H r) and decides the stop from it, as aypx_beta_x_kernel / pcg_aypx_beta_kernel do -- then
// x += alpha d ; d = beta d + r (PRE: d = beta d + m .* r) ; dc = conj(d).  rho of the previous iteration: history[iter - 1], with
// PRE the parity buffer rho2, so that work-group 0 may publish the new one in the same launch.
template <typename T, int BLOCK, bool VEC, bool PRE, bool GUARD>
__global__ __launch_bounds__(BLOCK) void herm_aypx_beta_x_kernel(int n, const T *__restrict__ rv, T *__restrict__ d, T *__restrict__ dc,
                                                                 T *__restrict__ xs, const T *__restrict__ m, long long mp, long long ld,
                                                                 const typename VT<T>::acc *__restrict__ part_rz,
                                                                 const typename VT<T>::acc *__restrict__ part_rr, int P, int K, int nrhs,
                                                                 const T *__restrict__ alpha, T *delta, T *beta, T *history,
                                                                 int history_cap, T *rho2, const int *iter, CgStop g) {
    using A = typename VT<T>::acc;
    __shared__ A red[BLOCK / kWave];
    __shared__ T beta_s;
    const int r = blockIdx.y;
    if (GUARD && g.live[r] == 0) {      // frozen before this iteration (live[] is written by the alpha step only)
        if (blockIdx.x == 0 && threadIdx.x == 0) stop_repeat_history(g, r, *iter, nrhs, history, history_cap);
        return;
    }
    {
        const A acc = thread_partials<BLOCK>((PRE ? part_rz : part_rr) + (long long)r * P, P, K);
        const A rho = block_sum<BLOCK>(acc, red);
        A rr = rho;
        if (PRE && blockIdx.x == 0) {
            const A acc2 = thread_partials<BLOCK>(part_rr + (long long)r * P, P, K);
            rr = block_sum<BLOCK>(acc2, red);
        }
        if (threadIdx.x == 0) {
            const int it = *iter;       // advanced by herm_alpha of this iteration
            const T rhoT = herm_real<T>(rho.x);
            const T rold = PRE ? rho2[(long long)((it - 1) & 1) * nrhs + r] : history[(long long)(it - 1) * nrhs + r];
            const T b = herm_ratio(rhoT, rold);
            beta_s = b;
            if (blockIdx.x == 0) {
                const T rrT = herm_real<T>(rr.x);
                beta[r] = b;
                delta[r] = rhoT;        // herm_alpha divides this by Re(d^H q)
                if (PRE) rho2[(long long)(it & 1) * nrhs + r] = rhoT;
                if (it < history_cap) history[(long long)it * nrhs + r] = rrT;
                if (GUARD) stop_decide(g, r, it, rrT);      // the updates below belong to this iteration whatever is decided
            }
        }
        __syncthreads();
    }
    const T bt = beta_s, al = alpha[r];
    rv += (long long)r * ld; d += (long long)r * ld; dc += (long long)r * ld; xs += (long long)r * ld;
    if (PRE) m += (long long)r * mp;
    constexpr int E = Pack<T>::N;
    const long long stride = (long long)gridDim.x * BLOCK;
    long long i0 = (long long)blockIdx.x * BLOCK + threadIdx.x;
    if (VEC) {
        const long long npack = n / E;
        for (long long i = i0; i < npack; i += stride) {
            const Pack<T> pr = ld_pack(rv + i * E);
            Pack<T> pd = ld_pack(d + i * E), px = ld_pack(xs + i * E), pm, pc;
            if (PRE) pm = ld_pack(m + i * E);
#pragma unroll
            for (int k = 0; k < E; ++k) {
                px.v[k] = vadd(px.v[k], vmul(al, pd.v[k]));
                pd.v[k] = PRE ? vadd(vmul(bt, pd.v[k]), vmul(pm.v[k], pr.v[k])) : vaypx(bt, pd.v[k], pr.v[k]);
                pc.v[k] = vconj(pd.v[k]);
            }
            st_pack(xs + i * E, px);
            st_pack(d + i * E, pd);
            st_pack(dc + i * E, pc);
        }
        i0 += npack * E;
    }
    for (long long i = i0; i < n; i += stride) {
        const T dv = d[i];
        xs[i] = vadd(xs[i], vmul(al, dv));
        const T dn = PRE ? vadd(vmul(bt, dv), vmul(m[i], rv[i])) : vaypx(bt, dv, rv[i]);
        d[i] = dn;
        dc[i] = vconj(dn);
    }
}

// ---- launchers: complex value types only ------------------------------------------------------------------------------------
#define CG_HERM_DISPATCH(dtype, FN, ...)                                                        \
    switch (dtype) {                                                                            \
    case CGAMD_C64: return FN<float2>(__VA_ARGS__);                                             \
    case CGAMD_C128: return FN<double2>(__VA_ARGS__);                                           \
    default: return fail(CGAMD_ERR_INVALID, "the conjugated recurrence is for the complex value types"); \
    }

template <typename T>
static int herm_init_impl(int n, const void *r, void *d, void *dc, const void *m, long long mp, long long ld, int nrhs, void *part_rz,
                          void *part_rr, int grid, bool vec, hipStream_t st) {
    dim3 g(grid, nrhs), blk(kBlock);
    using A = typename VT<T>::acc;
#define CG_HI(V, P) hipLaunchKernelGGL((herm_init_kernel<T, kBlock, V, P>), g, blk, 0, st, n, (const T *)r, (T *)d, (T *)dc, (const T *)m, mp, ld, \
                                       (A *)part_rz, (A *)part_rr)
    if (m) { if (vec) CG_HI(true, true); else CG_HI(false, true); }
    else if (vec) CG_HI(true, false);
    else CG_HI(false, false);
#undef CG_HI
    return check_launch("herm_init");
}
int launch_herm_init(int dtype, int n, const void *r, void *d, void *dc, const void *m, long long m_pitch, long long ld, int nrhs,
                     void *part_rz, void *part_rr, int grid, hipStream_t st) {
    if (n <= 0 || grid < 1) return fail(CGAMD_ERR_INVALID, "herm_init: empty launch");
    const bool vec = vec_ok(dtype, ld, nrhs, {r, d, dc, m}) && ((m_pitch * (long long)dtype_size(dtype)) & 15) == 0;
    CG_HERM_DISPATCH(dtype, herm_init_impl, n, r, d, dc, m, m_pitch, ld, nrhs, part_rz, part_rr, grid, vec, st);
}

template <typename T>
static int herm_delta0_impl(bool pre, const void *part_rz, const void *part_rr, int P, int nrhs, const CgScalars &sc, void *rho2,
                            hipStream_t st) {
    using A = typename VT<T>::acc;
#define CG_HD(P_) hipLaunchKernelGGL((herm_delta0_kernel<T, P_>), dim3(nrhs), dim3(kScalarBlock), 0, st, (const A *)part_rz, (const A *)part_rr, P, \
                                     nrhs, (T *)sc.delta, (T *)sc.history, (T *)rho2, sc.iter)
    if (pre) CG_HD(true); else CG_HD(false);
#undef CG_HD
    return check_launch("herm_delta0");
}
int launch_herm_delta0(int dtype, bool pre, const void *part_rz, const void *part_rr, int P, int nrhs, const CgScalars &sc, void *rho2,
                       hipStream_t st) {
    CG_HERM_DISPATCH(dtype, herm_delta0_impl, pre, part_rz, part_rr, P, nrhs, sc, rho2, st);
}

template <typename T>
static int herm_alpha_impl(const void *part_dq, int P, int nrhs, const CgScalars &sc, hipStream_t st, const CgStop *stop) {
    using A = typename VT<T>::acc;
    const CgStop none;
#define CG_HA(G) hipLaunchKernelGGL((herm_alpha_kernel<T, G>), dim3(nrhs), dim3(kScalarBlock), 0, st, (const A *)part_dq, P, sc.kdq, nrhs, \
                                    (const T *)sc.delta, (T *)sc.alpha, sc.iter, G ? *stop : none)
    if (stop) CG_HA(true); else CG_HA(false);
#undef CG_HA
    return check_launch("herm_alpha");
}
int launch_herm_alpha(int dtype, const void *part_dq, int P, int nrhs, const CgScalars &sc, hipStream_t st, const CgStop *stop) {
    CG_HERM_DISPATCH(dtype, herm_alpha_impl, part_dq, P, nrhs, sc, st, stop);
}

template <typename T>
static int herm_axpy_dot_impl(int n, const void *q, void *r, const void *m, long long mp, long long ld, const void *alpha, int nrhs,
                              void *part_rz, void *part_rr, int grid, bool vec, hipStream_t st, const CgStop *stop) {
    dim3 g(grid, nrhs), blk(kBlock);
    using A = typename VT<T>::acc;
    const CgStop none;
#define CG_HX(V, P, G) hipLaunchKernelGGL((herm_axpy_dot_kernel<T, kBlock, V, P, G>), g, blk, 0, st, n, (const T *)q, (T *)r, (const T *)m, mp, ld, \
                                          (const T *)alpha, (A *)part_rz, (A *)part_rr, G ? *stop : none)
    if (stop) {
        if (m) { if (vec) CG_HX(true, true, true); else CG_HX(false, true, true); }
        else if (vec) CG_HX(true, false, true);
        else CG_HX(false, false, true);
    } else if (m) { if (vec) CG_HX(true, true, false); else CG_HX(false, true, false); }
    else if (vec) CG_HX(true, false, false);
    else CG_HX(false, false, false);
#undef CG_HX
    return check_launch("herm_axpy_dot");
}
int launch_herm_axpy_dot(int dtype, int n, const void *q, void *r, const void *m, long long m_pitch, long long ld, const void *alpha,
                         int nrhs, void *part_rz, void *part_rr, int grid, hipStream_t st, const CgStop *stop) {
    if (n <= 0 || grid < 1) return fail(CGAMD_ERR_INVALID, "herm_axpy_dot: empty launch");
    const bool vec = vec_ok(dtype, ld, nrhs, {q, r, m}) && ((m_pitch * (long long)dtype_size(dtype)) & 15) == 0;
    CG_HERM_DISPATCH(dtype, herm_axpy_dot_impl, n, q, r, m, m_pitch, ld, alpha, nrhs, part_rz, part_rr, grid, vec, st, stop);
}

template <typename T>
static int herm_aypx_impl(int n, const void *r, void *d, void *dc, void *xs, const void *m, long long mp, long long ld, const void *part_rz,
                          const void *part_rr, int P, int nrhs, const CgScalars &sc, void *rho2, bool vec, hipStream_t st,
                          const CgStop *stop) {
    dim3 g(vec_grid(n, VT<T>::dtype, nrhs), nrhs), blk(kBlock);
    using A = typename VT<T>::acc;
    const CgStop none;
#define CG_HB(V, P_, G) hipLaunchKernelGGL((herm_aypx_beta_x_kernel<T, kBlock, V, P_, G>), g, blk, 0, st, n, (const T *)r, (T *)d, (T *)dc, (T *)xs, \
                                           (const T *)m, mp, ld, (const A *)part_rz, (const A *)part_rr, P, sc.krr, nrhs, (const T *)sc.alpha, \
                                           (T *)sc.delta, (T *)sc.beta, (T *)sc.history, sc.history_cap, (T *)rho2, (const int *)sc.iter, \
                                           G ? *stop : none)
    if (stop) {
        if (m) { if (vec) CG_HB(true, true, true); else CG_HB(false, true, true); }
        else if (vec) CG_HB(true, false, true);
        else CG_HB(false, false, true);
    } else if (m) { if (vec) CG_HB(true, true, false); else CG_HB(false, true, false); }
    else if (vec) CG_HB(true, false, false);
    else CG_HB(false, false, false);
#undef CG_HB
    return check_launch("herm_aypx_beta_x");
}
int launch_herm_aypx_beta_x(int dtype, int n, const void *r, void *d, void *dc, void *xs, const void *m, long long m_pitch, long long ld,
                            const void *part_rz, const void *part_rr, int P, int nrhs, const CgScalars &sc, void *rho2, hipStream_t st,
                            const CgStop *stop) {
    if (n <= 0) return CGAMD_OK;
    if (m && !rho2) return fail(CGAMD_ERR_INVALID, "herm_aypx_beta_x: a preconditioned step needs the rho buffer");
    const bool vec = vec_ok(dtype, ld, nrhs, {r, d, dc, xs, m}) && ((m_pitch * (long long)dtype_size(dtype)) & 15) == 0;
    CG_HERM_DISPATCH(dtype, herm_aypx_impl, n, r, d, dc, xs, m, m_pitch, ld, part_rz, part_rr, P, nrhs, sc, rho2, vec, st, stop);
}

}  // namespace cgamd
