/*
 * tests/native/p2x_probe.hip — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Probe kernels for the P2 exchange step's device code (csrc/sw_p2x_dev.h;
 * DESIGN.md §3.6), so that tests/test_gpu_p2x.py can feed it placements and
 * graphs of its own instead of what the placement cascade happens to leave.
 * Built by csrc/Makefile into lib/libp2x_probe.so with the product's flags;
 * never linked into libshockwave_amd.so.  It includes the product headers and
 * holds no copy of their code: each kernel is one 512-thread workgroup per
 * instance with the step's LDS layout (sw_p2x_lds, then the variable part at
 * SW_P2X_VAR_OFF, sized by sw_p2x_lds_bytes and passed as the launch's
 * dynamic LDS like sw_launch_p2x does).
 *
 *   p2x_probe_run         sw_p2x_block<SW_WAVES, 1> (the batch kernel's
 *                         instantiation) or <SW_WAVES, 8> (the sharded
 *                         engine's), pre = nullptr, on arrays in HBM
 *   p2x_probe_find_cycle  p2x_find_cycle on a given W, room and distances
 *   p2x_probe_edges       the step's set-up (sw_p2x_block's SETUP_ONLY form),
 *                         then p2x_load_size and one full p2x_build_w
 *
 * The host entry points take host arrays, return a hipError_t (0: success;
 * hipErrorInvalidValue for shapes the kernels cannot index) and synchronise.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../include/shockwave_amd.h"
#include "../../shockwave-replication_amd/csrc/sw_arith.h"
#include "../../shockwave-replication_amd/csrc/sw_block.h"
#include "../../shockwave-replication_amd/csrc/sw_device.h"
#include "../../shockwave-replication_amd/csrc/sw_p2x.h"
#include "../../shockwave-replication_amd/csrc/sw_p2x_dev.h"
#include "../../shockwave-replication_amd/csrc/sw_p2x_inst.h"

#define PROBE_CYC_STRIDE (SW_TMAX + 1) /* per-instance stride of dw and cyc */

/* Instance blockIdx.x: active jobs [off[i], off[i + 1]) of w, job, c, masks. */
template <int EMAX>
static __device__ __forceinline__ void probe_run(const int64_t* off, const int32_t* T, const int32_t* G,
                                                 int32_t* w, int32_t* job, double* c, uint64_t* masks,
                                                 int32_t* ncancel) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int inst = blockIdx.x;
    sw_p2x_lds* L = reinterpret_cast<sw_p2x_lds*>(smem);
    unsigned char* var = smem + SW_P2X_VAR_OFF;
    sw_blk blk;
    blk.X = &L->X;
    blk.par = 0;
    const int64_t o = off[inst];
    const int A = (int)(off[inst + 1] - o);
    sw_p2x_arrays X;
    X.cw = w + o;
    X.cj = job + o;
    X.cc = c + o;
    X.cm = masks + o;
    const int nc = sw_p2x_block<SW_WAVES, EMAX>(blk, L, var, X, A, T[inst], G[inst]);
    if (threadIdx.x == 0) ncancel[inst] = nc;
}

__global__ __launch_bounds__(SW_BLOCK, 8) void k_probe_run1(const int64_t* off, const int32_t* T,
                                                            const int32_t* G, int32_t* w, int32_t* job,
                                                            double* c, uint64_t* masks, int32_t* ncancel) {
    probe_run<1>(off, T, G, w, job, c, masks, ncancel);
}

__global__ __launch_bounds__(SW_BLOCK) void k_probe_run8(const int64_t* off, const int32_t* T,
                                                         const int32_t* G, int32_t* w, int32_t* job, double* c,
                                                         uint64_t* masks, int32_t* ncancel) {
    probe_run<8>(off, T, G, w, job, c, masks, ncancel);
}

/* Instance blockIdx.x: graph W[woff[i] + t·T + u] into the W region of LDS,
 * room and the distances into sw_p2x_lds, then p2x_find_cycle as the cancel
 * loop calls it (load size slot 0). */
__global__ __launch_bounds__(SW_BLOCK) void k_probe_find_cycle(const int32_t* T_, const int32_t* F_,
                                                               const int64_t* woff, const double* Wg,
                                                               const int32_t* room, double* dw,
                                                               const int32_t* warm, int32_t* len, int32_t* cyc) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int inst = blockIdx.x, tid = threadIdx.x;
    const int T = T_[inst], F = F_[inst];
    sw_p2x_lds* L = reinterpret_cast<sw_p2x_lds*>(smem);
    double* W = reinterpret_cast<double*>(smem + SW_P2X_VAR_OFF);
    for (int e = tid; e < T * T; e += SW_BLOCK) W[e] = Wg[woff[inst] + e];
    if (tid < T) L->room[tid] = room[(size_t)inst * SW_TMAX + tid];
    if (tid <= T) L->dw[0][tid] = dw[(size_t)inst * PROBE_CYC_STRIDE + tid];
    if (tid == 0) L->len = -1;
    __syncthreads();
    uint64_t acc[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    p2x_find_cycle(L, W, T, F, L->dw[0], warm[inst] != 0, acc);
    __syncthreads();
    const int n = L->len;
    if (tid == 0) len[inst] = n;
    if (tid < n) cyc[(size_t)inst * PROBE_CYC_STRIDE + tid] = L->cyc[tid];
    if (tid <= T) dw[(size_t)inst * PROBE_CYC_STRIDE + tid] = L->dw[0][tid];
}

/* Instance blockIdx.x: the set-up on its placement, then the edge costs of
 * load size F[i] as the cancel loop's first build makes them. */
template <int EMAX>
static __device__ __forceinline__ void probe_edges(const int64_t* off, const int32_t* T_, const int32_t* G,
                                                   const int32_t* F, int32_t* w, int32_t* job, double* c,
                                                   uint64_t* masks, const int64_t* woff, double* Wg,
                                                   int8_t* Wkg, double* delta) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int inst = blockIdx.x, tid = threadIdx.x;
    sw_p2x_lds* L = reinterpret_cast<sw_p2x_lds*>(smem);
    unsigned char* var = smem + SW_P2X_VAR_OFF;
    sw_blk blk;
    blk.X = &L->X;
    blk.par = 0;
    const int64_t o = off[inst];
    const int A = (int)(off[inst + 1] - o), T = T_[inst];
    sw_p2x_arrays X;
    X.cw = w + o;
    X.cj = job + o;
    X.cc = c + o;
    X.cm = masks + o;
    sw_p2x_state S;
    if (!sw_p2x_block<SW_WAVES, EMAX, true>(blk, L, var, X, A, T, G[inst], nullptr, nullptr, &S)) {
        if (tid == 0) delta[inst] = -1.0; /* skipped (uniform) */
        return;
    }
    p2x_load_size(L, S.K, F[inst]);
    __syncthreads();
    p2x_build_w<SW_BLOCK>(L, S.B, S.pc, S.W, S.Wk, T, S.delta, true);
    __syncthreads();
    for (int e = tid; e < T * T; e += SW_BLOCK) {
        Wg[woff[inst] + e] = S.W[e];
        Wkg[woff[inst] + e] = S.Wk[e];
    }
    if (tid == 0) delta[inst] = S.delta;
}

__global__ __launch_bounds__(SW_BLOCK, 8) void k_probe_edges1(const int64_t* off, const int32_t* T,
                                                              const int32_t* G, const int32_t* F, int32_t* w,
                                                              int32_t* job, double* c, uint64_t* masks,
                                                              const int64_t* woff, double* W, int8_t* Wk,
                                                              double* delta) {
    probe_edges<1>(off, T, G, F, w, job, c, masks, woff, W, Wk, delta);
}

__global__ __launch_bounds__(SW_BLOCK) void k_probe_edges8(const int64_t* off, const int32_t* T,
                                                           const int32_t* G, const int32_t* F, int32_t* w,
                                                           int32_t* job, double* c, uint64_t* masks,
                                                           const int64_t* woff, double* W, int8_t* Wk,
                                                           double* delta) {
    probe_edges<8>(off, T, G, F, w, job, c, masks, woff, W, Wk, delta);
}

namespace {

/* device copies of host arrays, freed on scope exit */
struct dev_pool {
    std::vector<void*> ptrs;
    hipError_t err = hipSuccess;
    ~dev_pool() {
        for (void* p : ptrs) (void)hipFree(p);
    }
    template <class V>
    V* up(const V* host, size_t n) {
        void* d = nullptr;
        if (err != hipSuccess) return nullptr;
        err = hipMalloc(&d, (n ? n : 1) * sizeof(V));
        if (err != hipSuccess) return nullptr;
        ptrs.push_back(d);
        if (n && host) err = hipMemcpy(d, host, n * sizeof(V), hipMemcpyHostToDevice);
        return static_cast<V*>(d);
    }
    template <class V>
    void down(V* host, const V* dev, size_t n) {
        if (err == hipSuccess && n) err = hipMemcpy(host, dev, n * sizeof(V), hipMemcpyDeviceToHost);
    }
};

} // namespace

/* the shapes the step's kernels can index: offsets, T, widths; the launch's LDS */
static bool probe_shapes_ok(int32_t count, const int64_t* offsets, const int32_t* T, const int32_t* w,
                            size_t* lds) {
    if (offsets[0] != 0) return false;
    *lds = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int64_t A = offsets[i + 1] - offsets[i];
        if (A < 0 || A > (int64_t)1 << 24 || T[i] < 0 || T[i] > SW_TMAX) return false;
        const size_t b = sw_p2x_lds_bytes((int)A, T[i]);
        *lds = b > *lds ? b : *lds;
    }
    const size_t n = (size_t)offsets[count];
    for (size_t a = 0; a < n; ++a)
        if (w[a] < 1 || w[a] > 255) return false; /* the width bitmap's range */
    return true;
}

/*
 * The step on count placements: instance i has the active jobs
 * [offsets[i], offsets[i + 1]) of w, job (ascending per instance), c and
 * masks (improved in place), T[i] rounds and G[i] GPUs; ncancel[i] out.
 * emax: 1 or 8, the rank sort's entries per thread (sw_p2x_block's EMAX).
 */
extern "C" int p2x_probe_run(int32_t count, const int64_t* offsets, const int32_t* T, const int32_t* G,
                             const int32_t* w, const int32_t* job, const double* c, uint64_t* masks,
                             int32_t* ncancel, int32_t emax) {
    if (count < 0 || (emax != 1 && emax != 8)) return (int)hipErrorInvalidValue;
    if (count == 0) return (int)hipSuccess;
    size_t lds = 0;
    if (!probe_shapes_ok(count, offsets, T, w, &lds)) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)offsets[count];
    dev_pool P;
    int64_t* d_off = P.up(offsets, (size_t)count + 1);
    int32_t* d_T = P.up(T, (size_t)count);
    int32_t* d_G = P.up(G, (size_t)count);
    int32_t* d_w = P.up(w, n);
    int32_t* d_job = P.up(job, n);
    double* d_c = P.up(c, n);
    uint64_t* d_m = P.up(masks, n);
    int32_t* d_nc = P.up((const int32_t*)nullptr, (size_t)count);
    if (P.err != hipSuccess) return (int)P.err;
    if (emax == 1)
        hipLaunchKernelGGL(k_probe_run1, dim3(count), dim3(SW_BLOCK), lds, 0, d_off, d_T, d_G, d_w, d_job,
                           d_c, d_m, d_nc);
    else
        hipLaunchKernelGGL(k_probe_run8, dim3(count), dim3(SW_BLOCK), lds, 0, d_off, d_T, d_G, d_w, d_job,
                           d_c, d_m, d_nc);
    P.err = hipGetLastError();
    if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
    P.down(masks, d_m, n);
    P.down(ncancel, d_nc, (size_t)count);
    return (int)P.err;
}

/*
 * p2x_find_cycle on count graphs: instance i has T[i] rounds, load size F[i],
 * W (its T·T costs, δ included, SW_P2X_NONE = no edge, instances packed one
 * after another), room[i·SW_TMAX + t], the distances dw[i·(SW_TMAX + 1) + x]
 * (in when warm[i], out always), and gets len[i] and cyc[i·(SW_TMAX + 1) + k].
 */
extern "C" int p2x_probe_find_cycle(int32_t count, const int32_t* T, const int32_t* F, const double* W,
                                    const int32_t* room, double* dw, const int32_t* warm, int32_t* len,
                                    int32_t* cyc) {
    if (count < 0) return (int)hipErrorInvalidValue;
    if (count == 0) return (int)hipSuccess;
    std::vector<int64_t> woff((size_t)count + 1, 0);
    int maxT = 0;
    for (int32_t i = 0; i < count; ++i) {
        if (T[i] < 2 || T[i] > SW_TMAX) return (int)hipErrorInvalidValue;
        woff[(size_t)i + 1] = woff[(size_t)i] + (int64_t)T[i] * T[i];
        maxT = T[i] > maxT ? T[i] : maxT;
    }
    const size_t lds = sw_p2x_lds_bytes(1, maxT); /* the variable part holds at least T·T costs */
    dev_pool P;
    int32_t* d_T = P.up(T, (size_t)count);
    int32_t* d_F = P.up(F, (size_t)count);
    int64_t* d_woff = P.up(woff.data(), (size_t)count + 1);
    double* d_W = P.up(W, (size_t)woff[(size_t)count]);
    int32_t* d_room = P.up(room, (size_t)count * SW_TMAX);
    double* d_dw = P.up(dw, (size_t)count * PROBE_CYC_STRIDE);
    int32_t* d_warm = P.up(warm, (size_t)count);
    int32_t* d_len = P.up((const int32_t*)nullptr, (size_t)count);
    int32_t* d_cyc = P.up((const int32_t*)nullptr, (size_t)count * PROBE_CYC_STRIDE);
    if (P.err != hipSuccess) return (int)P.err;
    P.err = hipMemset(d_cyc, 0xFF, (size_t)count * PROBE_CYC_STRIDE * sizeof(int32_t));
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k_probe_find_cycle, dim3(count), dim3(SW_BLOCK), lds, 0, d_T, d_F, d_woff, d_W, d_room,
                       d_dw, d_warm, d_len, d_cyc);
    P.err = hipGetLastError();
    if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
    P.down(dw, d_dw, (size_t)count * PROBE_CYC_STRIDE);
    P.down(len, d_len, (size_t)count);
    P.down(cyc, d_cyc, (size_t)count * PROBE_CYC_STRIDE);
    return (int)P.err;
}

/*
 * The step's set-up on count placements (as p2x_probe_run takes them) and one
 * full edge build for load size F[i]: W and Wk (instance i's T·T entries,
 * instances packed one after another; W with δ included) and delta[i] out
 * (−1, and W, Wk untouched, where the step is skipped).
 */
extern "C" int p2x_probe_edges(int32_t count, const int64_t* offsets, const int32_t* T, const int32_t* G,
                               const int32_t* F, const int32_t* w, const int32_t* job, const double* c,
                               const uint64_t* masks, double* W, int8_t* Wk, double* delta, int32_t emax) {
    if (count < 0 || (emax != 1 && emax != 8)) return (int)hipErrorInvalidValue;
    if (count == 0) return (int)hipSuccess;
    size_t lds = 0;
    if (!probe_shapes_ok(count, offsets, T, w, &lds)) return (int)hipErrorInvalidValue;
    std::vector<int64_t> woff((size_t)count + 1, 0);
    for (int32_t i = 0; i < count; ++i) {
        if (F[i] < 1) return (int)hipErrorInvalidValue;
        woff[(size_t)i + 1] = woff[(size_t)i] + (int64_t)T[i] * T[i];
    }
    const size_t n = (size_t)offsets[count], nw = (size_t)woff[(size_t)count];
    dev_pool P;
    int64_t* d_off = P.up(offsets, (size_t)count + 1);
    int32_t* d_T = P.up(T, (size_t)count);
    int32_t* d_G = P.up(G, (size_t)count);
    int32_t* d_F = P.up(F, (size_t)count);
    int32_t* d_w = P.up(w, n);
    int32_t* d_job = P.up(job, n);
    double* d_c = P.up(c, n);
    uint64_t* d_m = P.up(masks, n);
    int64_t* d_woff = P.up(woff.data(), (size_t)count + 1);
    double* d_W = P.up(W, nw);
    int8_t* d_Wk = P.up(Wk, nw);
    double* d_delta = P.up((const double*)nullptr, (size_t)count);
    if (P.err != hipSuccess) return (int)P.err;
    if (emax == 1)
        hipLaunchKernelGGL(k_probe_edges1, dim3(count), dim3(SW_BLOCK), lds, 0, d_off, d_T, d_G, d_F, d_w,
                           d_job, d_c, d_m, d_woff, d_W, d_Wk, d_delta);
    else
        hipLaunchKernelGGL(k_probe_edges8, dim3(count), dim3(SW_BLOCK), lds, 0, d_off, d_T, d_G, d_F, d_w,
                           d_job, d_c, d_m, d_woff, d_W, d_Wk, d_delta);
    P.err = hipGetLastError();
    if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
    P.down(W, d_W, nw);
    P.down(Wk, d_Wk, nw);
    P.down(delta, d_delta, (size_t)count);
    return (int)P.err;
}
