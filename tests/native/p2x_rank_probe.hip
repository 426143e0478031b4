/*
 * tests/native/p2x_rank_probe.hip — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Probe kernels for the P2 exchange step's set-up with a candidate rank order
 * (csrc/sw_p2x_dev.h, csrc/sw_p2x_rank.h), so that
 * tests/test_gpu_p2x_rank.py can hand it candidates of its own — the density
 * order, damaged orders, near ties — instead of what the pack leaves.  Built
 * by csrc/Makefile into lib/libp2x_rank_probe.so with the product's flags;
 * never linked into libshockwave_amd.so.  It includes the product headers and
 * holds no copy of their code: one 512-thread workgroup per instance with the
 * step's LDS layout, the per-job arrays in HBM.
 *
 *   p2x_rank_probe_setup  sw_p2x_block's SETUP_ONLY form, with or without a
 *                         candidate: the class header, ord, pc, the rank
 *                         bitsets, room, δ, and whether the candidate gave
 *                         the order
 *   p2x_rank_probe_run    the whole step with or without a candidate: masks
 *                         and the cancel count
 *
 * Instance i has the active jobs [offsets[i], offsets[i + 1]) of w, job, c
 * and masks; its candidate is the same range of cand (position words: the
 * job in the bits above 16), cand_n[i] positions (−1: no candidate) and jobs
 * below njobs[i].  The host entry points take host arrays, return a
 * hipError_t (0: success) and synchronise.
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

struct rank_probe_in {
    const int64_t* off;
    const int32_t *T, *G;
    int32_t *w, *job;
    double* c;
    uint64_t* masks;
    const uint32_t* cand;
    const int32_t *cand_n, *njobs;
};

__global__ __launch_bounds__(SW_BLOCK, 8) void k_rank_setup(rank_probe_in I, const int64_t* boff, int32_t* hdr,
                                                            int32_t* ord, double* pc, uint64_t* Bw, int32_t* room,
                                                            double* delta, int32_t* ranked) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int inst = blockIdx.x, tid = threadIdx.x;
    sw_p2x_lds* L = reinterpret_cast<sw_p2x_lds*>(smem);
    unsigned char* var = smem + SW_P2X_VAR_OFF;
    sw_blk blk;
    blk.X = &L->X;
    blk.par = 0;
    const int64_t o = I.off[inst];
    const int A = (int)(I.off[inst + 1] - o), T = I.T[inst];
    sw_p2x_arrays X;
    X.cw = I.w + o;
    X.cj = I.job + o;
    X.cc = I.c + o;
    X.cm = I.masks + o;
    sw_p2x_cand cd;
    cd.pos = I.cand + o;
    cd.n = I.cand_n[inst];
    cd.njobs = I.njobs[inst];
    sw_p2x_state S;
    if (!sw_p2x_block<SW_WAVES, 1, true>(blk, L, var, X, A, T, I.G[inst], nullptr, nullptr, &S,
                                         cd.n >= 0 ? &cd : nullptr)) {
        if (tid == 0) ranked[inst] = -1; /* skipped (uniform) */
        return;
    }
    const int K = S.K;
    int32_t* h = hdr + (size_t)inst * SW_P2X_HDR_INTS;
    if (tid == 0) {
        h[SW_P2X_HDR_K] = K;
        h[SW_P2X_HDR_A] = A;
        ranked[inst] = S.ranked;
        delta[inst] = S.delta;
    }
    if (tid < SW_P2X_KMAX) {
        const bool in = tid < K;
        h[SW_P2X_HDR_WC + tid] = in ? L->wc[tid] : 0;
        h[SW_P2X_HDR_M + tid] = in ? L->M[tid] : 0;
        h[SW_P2X_HDR_NW + tid] = in ? L->nw[tid] : 0;
        h[SW_P2X_HDR_BOFF + tid] = in ? L->boff[tid] : 0;
    }
    if (tid <= SW_P2X_KMAX) h[SW_P2X_HDR_OFF + tid] = tid <= K ? L->off[tid] : 0;
    for (int p = tid; p < A; p += SW_BLOCK) {
        ord[o + p] = S.ord[p];
        pc[o + p] = S.pc[p];
    }
    const int nwords = L->boff[K - 1] + L->nw[K - 1] * T;
    for (int i = tid; i < nwords; i += SW_BLOCK) Bw[boff[inst] + i] = S.B[i];
    if (tid < T) room[(size_t)inst * SW_TMAX + tid] = L->room[tid];
}

__global__ __launch_bounds__(SW_BLOCK, 8) void k_rank_run(rank_probe_in I, int32_t* ncancel) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int inst = blockIdx.x;
    sw_p2x_lds* L = reinterpret_cast<sw_p2x_lds*>(smem);
    unsigned char* var = smem + SW_P2X_VAR_OFF;
    sw_blk blk;
    blk.X = &L->X;
    blk.par = 0;
    const int64_t o = I.off[inst];
    const int A = (int)(I.off[inst + 1] - o);
    sw_p2x_arrays X;
    X.cw = I.w + o;
    X.cj = I.job + o;
    X.cc = I.c + o;
    X.cm = I.masks + o;
    sw_p2x_cand cd;
    cd.pos = I.cand + o;
    cd.n = I.cand_n[inst];
    cd.njobs = I.njobs[inst];
    const int nc = sw_p2x_block<SW_WAVES, 1>(blk, L, var, X, A, I.T[inst], I.G[inst], nullptr, nullptr, nullptr,
                                             cd.n >= 0 ? &cd : nullptr);
    if (threadIdx.x == 0) ncancel[inst] = nc;
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

/* the shapes the kernels can index; the launch's LDS */
bool shapes_ok(int32_t count, const int64_t* offsets, const int32_t* T, const int32_t* w, const int32_t* njobs,
               size_t* lds) {
    if (count < 0 || offsets[0] != 0) return false;
    *lds = 0;
    for (int32_t i = 0; i < count; ++i) {
        const int64_t A = offsets[i + 1] - offsets[i];
        if (A < 0 || A > (int64_t)1 << 24 || T[i] < 0 || T[i] > SW_TMAX || njobs[i] < 0 || njobs[i] > 65536)
            return false;
        const size_t b = sw_p2x_lds_bytes((int)A, T[i]);
        *lds = b > *lds ? b : *lds;
    }
    const size_t n = (size_t)offsets[count];
    for (size_t a = 0; a < n; ++a)
        if (w[a] < 1 || w[a] > 255) return false;
    return true;
}

rank_probe_in upload(dev_pool& P, int32_t count, const int64_t* offsets, const int32_t* T, const int32_t* G,
                     const int32_t* w, const int32_t* job, const double* c, const uint64_t* masks,
                     const uint32_t* cand, const int32_t* cand_n, const int32_t* njobs) {
    const size_t n = (size_t)offsets[count];
    rank_probe_in I;
    I.off = P.up(offsets, (size_t)count + 1);
    I.T = P.up(T, (size_t)count);
    I.G = P.up(G, (size_t)count);
    I.w = P.up(w, n);
    I.job = P.up(job, n);
    I.c = P.up(c, n);
    I.masks = P.up(masks, n);
    I.cand = P.up(cand, n);
    I.cand_n = P.up(cand_n, (size_t)count);
    I.njobs = P.up(njobs, (size_t)count);
    return I;
}

} // namespace

/*
 * The set-up on count placements.  Out: hdr[i·48 …] (the SW_P2X_HDR_ layout of
 * sw_p2x_dev.h, zero past K), ord and pc (per active position), the rank
 * bitsets (instance i's words from boff[i]; boff[count] words in all),
 * room[i·SW_TMAX + t], delta[i], ranked[i] (1: the candidate gave the order,
 * 0: the sort did, −1: the step is skipped and nothing else is written).
 */
extern "C" int p2x_rank_probe_setup(int32_t count, const int64_t* offsets, const int32_t* T, const int32_t* G,
                                    const int32_t* w, const int32_t* job, const double* c, const uint64_t* masks,
                                    const uint32_t* cand, const int32_t* cand_n, const int32_t* njobs,
                                    const int64_t* boff, int32_t* hdr, int32_t* ord, double* pc, uint64_t* Bw,
                                    int32_t* room, double* delta, int32_t* ranked) {
    if (count == 0) return (int)hipSuccess;
    size_t lds = 0;
    if (!shapes_ok(count, offsets, T, w, njobs, &lds)) return (int)hipErrorInvalidValue;
    for (int32_t i = 0; i < count; ++i) { /* room for every word the set-up can write */
        const int64_t A = offsets[i + 1] - offsets[i];
        if (boff[i + 1] - boff[i] < (int64_t)T[i] * ((A + 63) / 64 + SW_P2X_KMAX)) return (int)hipErrorInvalidValue;
    }
    const size_t n = (size_t)offsets[count], nb = (size_t)boff[count];
    dev_pool P;
    rank_probe_in I = upload(P, count, offsets, T, G, w, job, c, masks, cand, cand_n, njobs);
    int64_t* d_boff = P.up(boff, (size_t)count + 1);
    int32_t* d_hdr = P.up(hdr, (size_t)count * SW_P2X_HDR_INTS);
    int32_t* d_ord = P.up(ord, n);
    double* d_pc = P.up(pc, n);
    uint64_t* d_B = P.up(Bw, nb);
    int32_t* d_room = P.up(room, (size_t)count * SW_TMAX);
    double* d_delta = P.up(delta, (size_t)count);
    int32_t* d_ranked = P.up(ranked, (size_t)count);
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k_rank_setup, dim3(count), dim3(SW_BLOCK), lds, 0, I, d_boff, d_hdr, d_ord, d_pc, d_B,
                       d_room, d_delta, d_ranked);
    P.err = hipGetLastError();
    if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
    P.down(hdr, d_hdr, (size_t)count * SW_P2X_HDR_INTS);
    P.down(ord, d_ord, n);
    P.down(pc, d_pc, n);
    P.down(Bw, d_B, nb);
    P.down(room, d_room, (size_t)count * SW_TMAX);
    P.down(delta, d_delta, (size_t)count);
    P.down(ranked, d_ranked, (size_t)count);
    return (int)P.err;
}

/* The whole step on count placements: masks improved in place, ncancel[i] out. */
extern "C" int p2x_rank_probe_run(int32_t count, const int64_t* offsets, const int32_t* T, const int32_t* G,
                                  const int32_t* w, const int32_t* job, const double* c, uint64_t* masks,
                                  const uint32_t* cand, const int32_t* cand_n, const int32_t* njobs,
                                  int32_t* ncancel) {
    if (count == 0) return (int)hipSuccess;
    size_t lds = 0;
    if (!shapes_ok(count, offsets, T, w, njobs, &lds)) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)offsets[count];
    dev_pool P;
    rank_probe_in I = upload(P, count, offsets, T, G, w, job, c, masks, cand, cand_n, njobs);
    int32_t* d_nc = P.up(ncancel, (size_t)count);
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k_rank_run, dim3(count), dim3(SW_BLOCK), lds, 0, I, d_nc);
    P.err = hipGetLastError();
    if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
    P.down(masks, I.masks, n);
    P.down(ncancel, d_nc, (size_t)count);
    return (int)P.err;
}
