// Tridiagonal (line) preconditioner of the PCG recurrence: the reference PCG's spsolve branch (helmFE_var.py:561-562) for an M
// with entries only on |i - j| <= 1.  The solver factors M once (Thomas LU without pivoting, cgamd_solver_set_preconditioner_tridiag)
// and passes per row
//   nl[i] = -l_i            (l_i = M[i][i-1] / u_{i-1}; 0 at a segment start)
//   ne[i] = -w_i M[i][i+1]  (0 at a segment end)
//   w[i]  = 1 / u_i
// so that z = M^-1 r is the forward sweep y_i = r_i - l_i y_{i-1} followed by the backward sweep z_i = w_i y_i - w_i c_i z_{i+1}.
//
// pcg_tri_kernel takes the place of pcg_axpy2_dot2_kernel: per chunk of at most C = 256 R rows (R = 32 bytes of values per thread)
//   r -= alpha q (stored, r.r partial) ; forward sweep ; backward sweep ; z stored (q's storage, in place) ; r.z partial
// Both sweeps are first-order linear recurrences, i.e. compositions of affine maps v -> a v + b.  Each thread composes the maps of
// its R consecutive rows, a wave64 shuffle scan and then the four wave totals (LDS) give every thread the map of the rows before
// (forward) / after (backward) it, and the thread replays its rows.  nl = 0 at a segment start makes that row's map constant, so
// segment breaks need no special case.  Rows of a thread outside its chunk carry the identity map.  Every sum and scan runs in a
// fixed order and no atomics touch a value: results are run-to-run identical.
//
// Chunks (solver.cpp tri_plan) start at segment starts when every segment fits one chunk: nothing crosses a work-group.  Otherwise
// (a segment longer than C, e.g. a 1-D problem) the chunks are plain C-row slices and the sweep takes three launches:
//   MODE 1  r update (+ r.r), the forward scan with a zero carry-in and the chunk's maps: y_end = Pf y_in + Yf and
//           z_first = Pb z_in + Ub + Vb y_in (the backward sweep's response to the forward carry-in y_in as well)
//   carry   one thread per right-hand side walks the chunk maps in order: y_in and z_in of every chunk
//   MODE 2  the sweeps again with those carries (no update), z stored, r.z partial
// MODE 0 is the fused single launch.  UPD = false (set_rhs) skips the r update.
#include "cgamd_internal.h"
#include "device_types.h"
#include "device_mem.h"
#include "reduce_device.h"
#include "stop_device.h"
#include "launch_util.h"

namespace cgamd {

template <typename T> CG_DEV T vone();
template <> CG_DEV float vone<float>() { return 1.f; }
template <> CG_DEV double vone<double>() { return 1.; }
template <> CG_DEV float2 vone<float2>() { return make_float2(1.f, 0.f); }
template <> CG_DEV double2 vone<double2>() { return make_double2(1., 0.); }

CG_DEV float shfl_up_v(float v, int d) { return __shfl_up(v, d, kWave); }
CG_DEV double shfl_up_v(double v, int d) { return __shfl_up(v, d, kWave); }
CG_DEV float2 shfl_up_v(float2 v, int d) { return make_float2(__shfl_up(v.x, d, kWave), __shfl_up(v.y, d, kWave)); }
CG_DEV double2 shfl_up_v(double2 v, int d) { return make_double2(__shfl_up(v.x, d, kWave), __shfl_up(v.y, d, kWave)); }
CG_DEV float shfl_down_v(float v, int d) { return __shfl_down(v, d, kWave); }
CG_DEV double shfl_down_v(double v, int d) { return __shfl_down(v, d, kWave); }
CG_DEV float2 shfl_down_v(float2 v, int d) { return make_float2(__shfl_down(v.x, d, kWave), __shfl_down(v.y, d, kWave)); }
CG_DEV double2 shfl_down_v(double2 v, int d) { return make_double2(__shfl_down(v.x, d, kWave), __shfl_down(v.y, d, kWave)); }

template <typename T> constexpr int tri_rows() { return 32 / (int)sizeof(T); }
constexpr int kTriMaps = 7;     // per chunk and right-hand side: Pf, Yf, Pb, Ub, Vb, y_in, z_in

// R rows from row0 (a multiple of R); rows outside [lo, hi) get `fill`.  Whole 16-byte packs where all R rows are inside.
template <typename T, int R, bool VEC>
CG_DEV void ld_rows(const T *p, int row0, int lo, int hi, T fill, T (&o)[R]) {
    if (VEC && row0 >= lo && row0 + R <= hi) {
        constexpr int E = Pack<T>::N;
#pragma unroll
        for (int k = 0; k < R / E; ++k) {
            const Pack<T> pk = ld_pack(p + row0 + k * E);
#pragma unroll
            for (int j = 0; j < E; ++j) o[k * E + j] = pk.v[j];
        }
    } else {
#pragma unroll
        for (int i = 0; i < R; ++i) {
            o[i] = fill;
            if (row0 + i >= lo && row0 + i < hi) o[i] = p[row0 + i];
        }
    }
}
template <typename T, int R, bool VEC>
CG_DEV void st_rows(T *p, int row0, int lo, int hi, const T (&v)[R]) {
    if (VEC && row0 >= lo && row0 + R <= hi) {
        constexpr int E = Pack<T>::N;
#pragma unroll
        for (int k = 0; k < R / E; ++k) {
            Pack<T> pk;
#pragma unroll
            for (int j = 0; j < E; ++j) pk.v[j] = v[k * E + j];
            st_pack(p + row0 + k * E, pk);
        }
    } else {
#pragma unroll
        for (int i = 0; i < R; ++i)
            if (row0 + i >= lo && row0 + i < hi) p[row0 + i] = v[i];
    }
}

// grid = (G, nRHS); work-group g takes chunks g, g + G, ... and writes one partial per dot product: P = G partials per RHS.
// fpitch: values between the factors of consecutive right-hand sides (a batched handle: M_r of system r for right-hand side r); 0 =
// one M shared by all
// GUARD: the instantiation cgamd_solver_iterate_until launches; a right-hand side that has stopped keeps its r, z and partials
template <typename T, bool VEC, int MODE, bool UPD, bool GUARD = false>
__global__ __launch_bounds__(kBlock) void pcg_tri_kernel(const int *__restrict__ cstart, int nchunks, const T *__restrict__ nl,
                                                         const T *__restrict__ ne, const T *__restrict__ w, long long fpitch, const T *q, T *rv, T *z,
                                                         long long ld, const T *__restrict__ alpha, typename VT<T>::acc *__restrict__ part_rz,
                                                         typename VT<T>::acc *__restrict__ part_rr, T *__restrict__ maps, CgStop gd) {
    using A = typename VT<T>::acc;
    constexpr int R = tri_rows<T>(), NW = kBlock / kWave;
    if (GUARD && gd.stop[blockIdx.y] != 0) return;
    __shared__ T fa[NW], fb[NW], bp[NW], bu[NW], bv[NW];
    __shared__ A red[NW];
    const int rhs = blockIdx.y, lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const long long off = (long long)rhs * ld;
    rv += off; z += off; q += off;
    nl += rhs * fpitch; ne += rhs * fpitch; w += rhs * fpitch;
    const T one = vone<T>(), zero = vzero<T>();
    const T al = UPD ? alpha[rhs] : zero;
    A arz = vzero<A>(), arr = vzero<A>();
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int cs = cstart[c], ce = cstart[c + 1];
        const int row0 = cs / R * R + (int)threadIdx.x * R;
        T r[R], a[R], e[R], wy[R], wg[R];
        ld_rows<T, R, VEC>(rv, row0, cs, ce, zero, r);
        ld_rows<T, R, true>(nl, row0, cs, ce, one, a);
        ld_rows<T, R, true>(ne, row0, cs, ce, one, e);
        ld_rows<T, R, true>(w, row0, cs, ce, zero, wy);
        if (UPD) {
            T qq[R];
            ld_rows<T, R, VEC>(q, row0, cs, ce, zero, qq);
#pragma unroll
            for (int i = 0; i < R; ++i) r[i] = vsub(r[i], vmul(al, qq[i]));
            st_rows<T, R, VEC>(rv, row0, cs, ce, r);
        }
        if (MODE != 2) {
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (row0 + i >= cs && row0 + i < ce) arr = vadd(arr, to_acc(vmul(r[i], r[i])));
        }
        // ---- forward sweep y_i = nl_i y_{i-1} + r_i: the thread's map, inclusive wave scan, wave totals
        T FA = one, FB = zero;
#pragma unroll
        for (int i = 0; i < R; ++i) { FB = vadd(vmul(a[i], FB), r[i]); FA = vmul(a[i], FA); }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const T a2 = shfl_up_v(FA, d), b2 = shfl_up_v(FB, d);
            if (lane >= d) { FB = vadd(vmul(FA, b2), FB); FA = vmul(FA, a2); }
        }
        T XA = shfl_up_v(FA, 1), XB = shfl_up_v(FB, 1);       // exclusive: the rows of the lanes before
        if (lane == 0) { XA = one; XB = zero; }
        if (lane == kWave - 1) { fa[wv] = FA; fb[wv] = FB; }
        __syncthreads();
        {
            T PA = one, PB = zero;                               // the waves before, in order
            for (int k = 0; k < wv; ++k) { PB = vadd(vmul(fa[k], PB), fb[k]); PA = vmul(fa[k], PA); }
            XB = vadd(vmul(XA, PB), XB);
            XA = vmul(XA, PA);
        }
        T carry_f = zero, carry_b = zero;
        T *mp = maps + ((long long)rhs * nchunks + c) * kTriMaps;
        if (MODE == 2) { carry_f = mp[5]; carry_b = mp[6]; }
        T y = MODE == 2 ? vadd(vmul(XA, carry_f), XB) : XB;    // y of the row before the thread's first
        T g = XA;                                               // MODE 1: its gain on the chunk's carry-in
#pragma unroll
        for (int i = 0; i < R; ++i) {
            y = vadd(vmul(a[i], y), r[i]);
            if (MODE == 1) { g = vmul(a[i], g); wg[i] = vmul(wy[i], g); }
            wy[i] = vmul(wy[i], y);
        }
        // ---- backward sweep z_i = ne_i z_{i+1} + w_i y_i (MODE 1: + w_i g_i y_in): thread map from its last row, suffix scan
        T BP = one, BU = zero, BV = zero;
#pragma unroll
        for (int i = R - 1; i >= 0; --i) {
            BU = vadd(vmul(e[i], BU), wy[i]);
            if (MODE == 1) BV = vadd(vmul(e[i], BV), wg[i]);
            BP = vmul(e[i], BP);
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            const T p2 = shfl_down_v(BP, d), u2 = shfl_down_v(BU, d);
            const T v2 = MODE == 1 ? shfl_down_v(BV, d) : zero;
            if (lane + d < kWave) {
                BU = vadd(vmul(BP, u2), BU);
                if (MODE == 1) BV = vadd(vmul(BP, v2), BV);
                BP = vmul(BP, p2);
            }
        }
        T YP = shfl_down_v(BP, 1), YU = shfl_down_v(BU, 1);     // exclusive: the rows of the lanes after
        if (lane == kWave - 1) { YP = one; YU = zero; }
        if (lane == 0) { bp[wv] = BP; bu[wv] = BU; if (MODE == 1) bv[wv] = BV; }
        __syncthreads();
        if (MODE == 1) {
            if (threadIdx.x == 0) {                             // the chunk's maps
                T TA = one, TB = zero, TP = one, TU = zero, TV = zero;
                for (int k = 0; k < NW; ++k) { TB = vadd(vmul(fa[k], TB), fb[k]); TA = vmul(fa[k], TA); }
                for (int k = NW - 1; k >= 0; --k) {
                    TU = vadd(vmul(bp[k], TU), bu[k]);
                    TV = vadd(vmul(bp[k], TV), bv[k]);
                    TP = vmul(bp[k], TP);
                }
                mp[0] = TA; mp[1] = TB; mp[2] = TP; mp[3] = TU; mp[4] = TV;
            }
        } else {
            T SP = one, SU = zero;                               // the waves after, from the last one
            for (int k = NW - 1; k > wv; --k) { SU = vadd(vmul(bp[k], SU), bu[k]); SP = vmul(bp[k], SP); }
            YU = vadd(vmul(YP, SU), YU);
            YP = vmul(YP, SP);
            T zn = MODE == 2 ? vadd(vmul(YP, carry_b), YU) : YU;   // z of the row after the thread's last
            T zz[R];
#pragma unroll
            for (int i = R - 1; i >= 0; --i) { zn = vadd(vmul(e[i], zn), wy[i]); zz[i] = zn; }
            st_rows<T, R, VEC>(z, row0, cs, ce, zz);
#pragma unroll
            for (int i = 0; i < R; ++i)
                if (row0 + i >= cs && row0 + i < ce) arz = vadd(arz, to_acc(vmul(r[i], zz[i])));
        }
        __syncthreads();      // fa / bp of this chunk are read above; the next chunk writes them
    }
    if (MODE != 1) {
        const A trz = block_sum<kBlock>(arz, red);
        if (threadIdx.x == 0) part_rz[(long long)rhs * gridDim.x + blockIdx.x] = trz;
    }
    if (MODE != 2) {
        const A trr = block_sum<kBlock>(arr, red);
        if (threadIdx.x == 0) part_rr[(long long)rhs * gridDim.x + blockIdx.x] = trr;
    }
}

// chunk carries in order: y_in[c + 1] = Pf[c] y_in[c] + Yf[c]; then from the last chunk z_in[c - 1] = Pb[c] z_in[c] + Ub[c] + Vb[c] y_in[c]
template <typename T>
__global__ __launch_bounds__(64) void pcg_tri_carry_kernel(int nchunks, int nrhs, T *maps) {
    const int rhs = blockIdx.x * 64 + threadIdx.x;
    if (rhs >= nrhs) return;
    T *m = maps + (long long)rhs * nchunks * kTriMaps;
    T v = vzero<T>();
    for (int c = 0; c < nchunks; ++c) {
        T *mc = m + (long long)c * kTriMaps;
        mc[5] = v;
        v = vadd(vmul(mc[0], v), mc[1]);
    }
    T u = vzero<T>();
    for (int c = nchunks - 1; c >= 0; --c) {
        T *mc = m + (long long)c * kTriMaps;
        mc[6] = u;
        u = vadd(vadd(vmul(mc[2], u), mc[3]), vmul(mc[4], mc[5]));
    }
}

int tri_chunk_rows(int dtype) { return kBlock * (32 / (int)dtype_size(dtype)); }
int tri_maps_values(int nchunks, int nrhs) { return nchunks * nrhs * kTriMaps; }

template <typename T>
static int tri_impl(const TriLaunch &t, bool update, const void *q, void *r, void *z, long long ld, const void *alpha, int nrhs,
                    void *part_rz, void *part_rr, bool vec, hipStream_t st, const CgStop *stop) {
    using A = typename VT<T>::acc;
    const dim3 g(t.grid, nrhs), blk(kBlock);
    const T *nl = (const T *)t.nl, *ne = (const T *)t.ne, *w = (const T *)t.w;
    T *maps = (T *)t.maps;
    const CgStop none;
#define CG_TRIG(V, M, U, G) hipLaunchKernelGGL((pcg_tri_kernel<T, V, M, U, G>), g, blk, 0, st, t.cstart, t.nchunks, nl, ne, w, t.fpitch, (const T *)q, (T *)r, \
                                               (T *)z, ld, (const T *)alpha, (A *)part_rz, (A *)part_rr, maps, G ? *stop : none)
#define CG_TRI(V, M, U) CG_TRIG(V, M, U, false)
    if (stop && update) {       // the loop of cgamd_solver_iterate_until (the carry launch in between only rewrites a frozen column's chunk maps)
        if (!t.longform) {
            if (vec) CG_TRIG(true, 0, true, true); else CG_TRIG(false, 0, true, true);
            return check_launch("pcg_tri");
        }
        if (vec) CG_TRIG(true, 1, true, true); else CG_TRIG(false, 1, true, true);
        if (int rc = check_launch("pcg_tri maps")) return rc;
        hipLaunchKernelGGL((pcg_tri_carry_kernel<T>), dim3((nrhs + 63) / 64), dim3(64), 0, st, t.nchunks, nrhs, maps);
        if (int rc = check_launch("pcg_tri carry")) return rc;
        if (vec) CG_TRIG(true, 2, false, true); else CG_TRIG(false, 2, false, true);
        return check_launch("pcg_tri apply");
    }
    if (!t.longform) {
        if (update) { if (vec) CG_TRI(true, 0, true); else CG_TRI(false, 0, true); }
        else { if (vec) CG_TRI(true, 0, false); else CG_TRI(false, 0, false); }
        return check_launch("pcg_tri");
    }
    if (update) { if (vec) CG_TRI(true, 1, true); else CG_TRI(false, 1, true); }
    else { if (vec) CG_TRI(true, 1, false); else CG_TRI(false, 1, false); }
    if (int rc = check_launch("pcg_tri maps")) return rc;
    hipLaunchKernelGGL((pcg_tri_carry_kernel<T>), dim3((nrhs + 63) / 64), dim3(64), 0, st, t.nchunks, nrhs, maps);
    if (int rc = check_launch("pcg_tri carry")) return rc;
    if (vec) CG_TRI(true, 2, false); else CG_TRI(false, 2, false);
#undef CG_TRI
#undef CG_TRIG
    return check_launch("pcg_tri apply");
}
int launch_pcg_tri(int dtype, const TriLaunch &t, bool update, const void *q, void *r, void *z, long long ld, const void *alpha, int nrhs,
                   void *part_rz, void *part_rr, hipStream_t st, const CgStop *stop) {
    const bool vec = vec_ok(dtype, ld, nrhs, {q, r, z});
    CG_DISPATCH(dtype, tri_impl, t, update, q, r, z, ld, alpha, nrhs, part_rz, part_rr, vec, st, stop);
}

}  // namespace cgamd
