// Host side of the tolerance stop of the launched loops (StopRun, cgamd_internal.h): what cgamd_solver_iterate_until and
// cgamd_dist_iterate_until share.  The guarded kernels are in stop_device.h; which launches an iteration is made of is the owner's
// business (enqueue_iteration of solver.cpp and dist.cpp, with the record's view).
#include <algorithm>

#include "cgamd_internal.h"

namespace cgamd {

// the device record: [nactive, pad x3] [tol: nr doubles] [stop: nr ints] [live: nr ints]
static size_t rec_bytes(int nr) { return 16 + (size_t)nr * 16; }
// the pinned block: [0..1] active counts, [2] the owner's word, [3 ..] stop[], then the record's image, 8-byte aligned
static size_t pin_ints(int nr) { return 4 + (size_t)nr + (size_t)(nr & 1); }

int stop_run_alloc(StopRun &sr, int nr) {
    if (!sr.rec) {
        hipError_t e = hipMalloc(&sr.rec, rec_bytes(nr));
        if (e != hipSuccess) return fail(CGAMD_ERR_ALLOC, std::string("hipMalloc(stop record): ") + hipGetErrorString(e));
        char *base = static_cast<char *>(sr.rec);
        sr.view.nactive = reinterpret_cast<int *>(base);
        sr.view.tol = reinterpret_cast<const double *>(base + 16);
        sr.view.stop = reinterpret_cast<int *>(base + 16 + (size_t)nr * 8);
        sr.view.live = sr.view.stop + nr;
        sr.nr = nr;
    }
    if (!sr.pin) {
        CG_HIP(hipHostMalloc((void **)&sr.pin, pin_ints(nr) * 4 + rec_bytes(nr), hipHostMallocDefault));
        sr.stopped = sr.pin + 3;
        std::fill(sr.stopped, sr.stopped + nr, 0);
    }
    for (hipEvent_t &e : sr.ev)
        if (!e) CG_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return CGAMD_OK;
}

int stop_run_arm(StopRun &sr, const double *tol, int nTol, hipStream_t st) {
    const int nr = sr.nr;
    char *img = reinterpret_cast<char *>(sr.pin + pin_ints(nr));
    double *tl = reinterpret_cast<double *>(img + 16);
    for (int r = 0; r < nr; ++r) tl[r] = tol[nTol == 1 ? 0 : r];
    if (sr.armed) {             // (a stopped right-hand side stays stopped whatever the new tolerances are)
        CG_HIP(hipMemcpyAsync(static_cast<char *>(sr.rec) + 16, tl, (size_t)nr * 8, hipMemcpyHostToDevice, st));
        return CGAMD_OK;
    }
    int *hd = reinterpret_cast<int *>(img), *sp = reinterpret_cast<int *>(img + 16 + (size_t)nr * 8);
    hd[0] = nr; hd[1] = hd[2] = hd[3] = 0;
    for (int r = 0; r < nr; ++r) { sp[r] = 0; sp[nr + r] = 1; }
    CG_HIP(hipMemcpyAsync(sr.rec, img, rec_bytes(nr), hipMemcpyHostToDevice, st));
    std::fill(sr.stopped, sr.stopped + nr, 0);
    sr.armed = true;
    return CGAMD_OK;
}

int stop_run_chunks(StopRun &sr, int maxIterations, int chunk, hipStream_t st, const std::function<int(int)> &enqueue) {
    volatile int *count = sr.pin;
    sr.enqueued = 0;
    sr.active = true;
    for (int c = 0; sr.enqueued < maxIterations && sr.active; ++c) {
        const int len = std::min(chunk, maxIterations - sr.enqueued);
        if (int rc = enqueue(len)) return rc;
        sr.enqueued += len;
        CG_HIP(hipMemcpyAsync(sr.pin + (c & 1), sr.view.nactive, sizeof(int), hipMemcpyDeviceToHost, st));
        CG_HIP(hipEventRecord(sr.ev[c & 1], st));
        if (c > 0) {            // chunk c is in the stream: now the count chunk c - 1 left
            CG_HIP(hipEventSynchronize(sr.ev[(c - 1) & 1]));
            sr.active = count[(c - 1) & 1] != 0;
        }
    }
    return CGAMD_OK;
}

int stop_run_read(StopRun &sr, hipStream_t st) {
    CG_HIP(hipMemcpyAsync(sr.stopped, sr.view.stop, sizeof(int) * (size_t)sr.nr, hipMemcpyDeviceToHost, st));
    return CGAMD_OK;
}

void stop_run_free(StopRun &sr) {
    if (sr.rec) (void)hipFree(sr.rec);
    if (sr.pin) (void)hipHostFree(sr.pin);
    for (hipEvent_t e : sr.ev)
        if (e) (void)hipEventDestroy(e);
    sr = StopRun();
}

}  // namespace cgamd
