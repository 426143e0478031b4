/*
 * tests/native/pack_probe.hip — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Probe kernels for the placement's round loop (csrc/sw_pack.h; DESIGN.md
 * §3.3) and the wave / block primitives it stands on (csrc/sw_block.h), so
 * that tests/test_gpu_pack.py can run every compiled form of the loop on
 * positions of its own, at any size the form can hold, instead of only at the
 * sizes at which a whole plan solve selects it.  Built by csrc/Makefile into
 * lib/libpack_probe.so with the product's flags; never linked into
 * libshockwave_amd.so.  It includes the product headers and holds no copy of
 * their code.
 *
 *   pack_probe_block  sw_pack_rounds<E, sw_blk_t<SW_WAVES>> on 512 threads,
 *                     E = 2 (the plan kernel), 4, 8, 20, 32, 64 (sw_shard.hip)
 *   pack_probe_wave   sw_pack_rounds_wave<E1> on 64 threads, the round masks
 *                     in LDS as k_pack_rounds_wave has them, E1 = 2, 4, 6, 8
 *                     (sw_pack_rounds_one, sw_rounds_kernel), 16, 32, 64
 *   pack_probe_one    sw_pack_rounds_one<MULTI> on 512 threads, one position
 *                     per thread staged through a 6 KB block
 *   pack_probe_room   sw_pack_room for every round of a capacity row, with the
 *                     row's sw_pack_caps_base and with cbase = −1
 *   pack_probe_prims  the wave primitives on 64-lane vectors and the block
 *                     primitives on 512 values
 *
 * One workgroup per case, one launch per call.  A case is the positions
 * [off[i], off[i + 1]) of st, already in placement order (st = r | w << 8),
 * T[i] rounds, G[i] GPUs, the capacity row caps[64·i …] and has[i] (0: every
 * round holds G[i]).  All 64 words of a row are copied to LDS, so what the
 * caller leaves past T is what the loop would read there.  The host entry
 * points take host arrays, return a hipError_t (0: success;
 * hipErrorInvalidValue for shapes the kernels cannot index) and synchronise.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "../../shockwave-replication_amd/csrc/sw_block.h"
#include "../../shockwave-replication_amd/csrc/sw_pack.h"

#define PROBE_RMAX 64           /* rounds a position may carry: the histogram's bins */
#define PROBE_CAPMAX (1 << 24)  /* capacities and G: 64 of them sum inside 32 bits */

struct probe_case {
    int64_t o;
    int A, T, G;
    bool has;
};

static __device__ __forceinline__ probe_case probe_open(const int64_t* off, const int32_t* T, const int32_t* G,
                                                        const int32_t* caps, const int32_t* has,
                                                        int32_t* capsL) {
    const int inst = blockIdx.x;
    probe_case c;
    c.o = off[inst];
    c.A = (int)(off[inst + 1] - c.o);
    c.T = T[inst];
    c.G = G[inst];
    c.has = has[inst] != 0;
    if (threadIdx.x < 64) capsL[threadIdx.x] = caps[(size_t)inst * 64 + threadIdx.x];
    return c;
}

template <int E>
__global__ __launch_bounds__(SW_BLOCK) void k_probe_block(const int64_t* off, const int32_t* T,
                                                          const int32_t* G, const int32_t* caps,
                                                          const int32_t* has, const uint32_t* sti,
                                                          uint64_t* mko, uint32_t* sto) {
    __shared__ sw_xchg X;
    __shared__ sw_pack_lds PL;
    __shared__ int32_t capsL[64];
    sw_blk blk;
    blk.X = &X;
    blk.par = 0;
    const int tid = threadIdx.x;
    const probe_case c = probe_open(off, T, G, caps, has, capsL);
    uint32_t st[E];
    uint64_t mk[E];
#pragma unroll
    for (int i = 0; i < E; ++i) st[i] = E * tid + i < c.A ? sti[c.o + E * tid + i] : 0u;
    __syncthreads(); /* capsL */
    sw_pack_rounds<E>(blk, &PL, c.A, c.T, c.G, st, mk, c.has ? capsL : nullptr);
#pragma unroll
    for (int i = 0; i < E; ++i)
        if (E * tid + i < c.A) {
            mko[c.o + E * tid + i] = mk[i];
            sto[c.o + E * tid + i] = st[i];
        }
}

template <int E1>
__global__ __launch_bounds__(64) void k_probe_wave(const int64_t* off, const int32_t* T, const int32_t* G,
                                                   const int32_t* caps, const int32_t* has,
                                                   const uint32_t* sti, uint64_t* mko, uint32_t* sto) {
    __shared__ sw_pack_lds PL;
    __shared__ int32_t capsL[64];
    __shared__ uint64_t xmk[64 * E1];
    const int lane = lane_id();
    const probe_case c = probe_open(off, T, G, caps, has, capsL);
    uint32_t st[E1];
#pragma unroll
    for (int i = 0; i < E1; ++i) st[i] = E1 * lane + i < c.A ? sti[c.o + E1 * lane + i] : 0u;
    wave_sync(); /* capsL */
    sw_pack_rounds_wave<E1>(&PL, c.T, c.G, st, xmk, c.has ? capsL : nullptr);
#pragma unroll
    for (int i = 0; i < E1; ++i)
        if (E1 * lane + i < c.A) {
            mko[c.o + E1 * lane + i] = xmk[E1 * lane + i];
            sto[c.o + E1 * lane + i] = st[i];
        }
}

template <bool MULTI>
__global__ __launch_bounds__(SW_BLOCK) void k_probe_one(const int64_t* off, const int32_t* T, const int32_t* G,
                                                        const int32_t* caps, const int32_t* has,
                                                        const uint32_t* sti, uint64_t* mko, uint32_t* sto) {
    __shared__ sw_pack_lds PL;
    __shared__ int32_t capsL[64];
    __shared__ uint64_t xs[(SW_BLOCK * 4 + SW_BLOCK * 8) / 8]; /* 512 states, 512 masks: 6 KB */
    const int tid = threadIdx.x;
    const probe_case c = probe_open(off, T, G, caps, has, capsL);
    uint32_t st1 = tid < c.A ? sti[c.o + tid] : 0u;
    uint64_t mk1 = 0;
    __syncthreads(); /* capsL */
    sw_pack_rounds_one<MULTI>(&PL, c.A, c.T, c.G, st1, mk1, xs, c.has ? capsL : nullptr);
    if (tid < c.A) {
        mko[c.o + tid] = mk1;
        sto[c.o + tid] = st1;
    }
}

/* Case blockIdx.x, round t, lane m: room[(inst·64 + t)·64 + m] with the row's
 * cbase (ra) and with cbase = −1 (rb); cb[inst] that cbase. */
__global__ __launch_bounds__(64) void k_probe_room(const int32_t* T, const int32_t* G, const int32_t* caps,
                                                   const int32_t* has, int32_t* ra, int32_t* rb, int32_t* cb) {
    __shared__ int32_t capsL[64];
    const int inst = blockIdx.x, lane = lane_id();
    capsL[lane] = caps[(size_t)inst * 64 + lane];
    wave_sync();
    const int32_t* cp = has[inst] ? capsL : nullptr;
    const int Tn = T[inst], Gn = G[inst];
    const int32_t cbase = sw_pack_caps_base(cp, Tn);
    if (lane == 0) cb[inst] = cbase;
    for (int t = 0; t < Tn; ++t) {
        const size_t at = ((size_t)inst * 64 + t) * 64 + lane;
        ra[at] = sw_pack_room(cp, t, Tn - t, Gn, cbase);
        rb[at] = sw_pack_room(cp, t, Tn - t, Gn);
    }
}

/* Vector blockIdx.x: out[(v·6 + k)·64 + lane], k = 0 sort, 5 max, 4 min of vs;
 * 1 inclusive scan, 2 suffix scan, 3 sum of va. */
__global__ __launch_bounds__(64) void k_probe_wave_prims(const int32_t* vs, const int32_t* va, int32_t* out) {
    const int lane = lane_id();
    const size_t v = blockIdx.x;
    const int32_t s = vs[v * 64 + lane], a = va[v * 64 + lane];
    int32_t* o = out + v * 6 * 64 + lane;
    o[0 * 64] = wave_sort_asc_i32(s);
    o[1 * 64] = wave_incscan_i32(a);
    o[2 * 64] = wave_sufscan_i32(a);
    o[3 * 64] = wave_sum_i32(a);
    o[4 * 64] = wave_min_i32(s);
    o[5 * 64] = wave_max_i32(s);
}

/* Pair blockIdx.x of 512-value vectors a, b: out[(v·8 + k)·512 + tid], k = 0, 1
 * exscan(a) and its total, 2, 3 exscan(b) and its total, 4, 5 sum32(a), sum32(b),
 * 6, 7 min32(a), min32(b) — each primitive twice in a row, once per slot set. */
__global__ __launch_bounds__(SW_BLOCK) void k_probe_block_prims(const int32_t* va, const int32_t* vb,
                                                                int32_t* out) {
    __shared__ sw_xchg X;
    sw_blk blk;
    blk.X = &X;
    blk.par = 0;
    const int tid = threadIdx.x;
    const size_t v = blockIdx.x;
    const int32_t a = va[v * SW_BLOCK + tid], b = vb[v * SW_BLOCK + tid];
    int32_t* o = out + v * 8 * SW_BLOCK + tid;
    int32_t tot;
    o[0 * SW_BLOCK] = blk.exscan(a, tot);
    o[1 * SW_BLOCK] = tot;
    o[2 * SW_BLOCK] = blk.exscan(b, tot);
    o[3 * SW_BLOCK] = tot;
    o[4 * SW_BLOCK] = blk.sum32(a);
    o[5 * SW_BLOCK] = blk.sum32(b);
    o[6 * SW_BLOCK] = blk.min32(a);
    o[7 * SW_BLOCK] = blk.min32(b);
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

/* rounds, G and the capacity rows in use of count cases inside what the loop indexes */
bool rows_ok(int32_t count, const int32_t* T, const int32_t* G, const int32_t* caps, const int32_t* has) {
    for (int32_t i = 0; i < count; ++i) {
        if (T[i] < 0 || T[i] > 64 || G[i] < 0 || G[i] > PROBE_CAPMAX) return false;
        for (int t = 0; has[i] && t < T[i]; ++t)
            if (caps[(size_t)i * 64 + t] < 0 || caps[(size_t)i * 64 + t] > PROBE_CAPMAX) return false;
    }
    return true;
}

/* every case has at most amax positions, each with r ≤ 64 and no bits above w */
bool cases_ok(int32_t count, const int64_t* off, const int32_t* T, const int32_t* G, const int32_t* caps,
              const int32_t* has, const uint32_t* st, int64_t amax) {
    if (off[0] != 0 || !rows_ok(count, T, G, caps, has)) return false;
    for (int32_t i = 0; i < count; ++i)
        if (off[i + 1] < off[i] || off[i + 1] - off[i] > amax) return false;
    for (int64_t p = 0; p < off[count]; ++p)
        if ((st[p] & 0xFFu) > PROBE_RMAX || (st[p] >> 16) != 0) return false;
    return true;
}

using loop_kernel = void (*)(const int64_t*, const int32_t*, const int32_t*, const int32_t*, const int32_t*,
                             const uint32_t*, uint64_t*, uint32_t*);

int run_loop(loop_kernel k, int threads, int64_t amax, int32_t count, const int64_t* off, const int32_t* T,
             const int32_t* G, const int32_t* caps, const int32_t* has, const uint32_t* st, uint64_t* mk,
             uint32_t* sto) {
    if (count < 0) return (int)hipErrorInvalidValue;
    if (count == 0) return (int)hipSuccess;
    if (!cases_ok(count, off, T, G, caps, has, st, amax)) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)off[count];
    dev_pool P;
    int64_t* d_off = P.up(off, (size_t)count + 1);
    int32_t* d_T = P.up(T, (size_t)count);
    int32_t* d_G = P.up(G, (size_t)count);
    int32_t* d_caps = P.up(caps, (size_t)count * 64);
    int32_t* d_has = P.up(has, (size_t)count);
    uint32_t* d_st = P.up(st, n);
    uint64_t* d_mk = P.up((const uint64_t*)nullptr, n);
    uint32_t* d_sto = P.up((const uint32_t*)nullptr, n);
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k, dim3(count), dim3(threads), 0, 0, d_off, d_T, d_G, d_caps, d_has, d_st, d_mk, d_sto);
    P.err = hipGetLastError();
    if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
    P.down(mk, d_mk, n);
    P.down(sto, d_sto, n);
    return (int)P.err;
}

} // namespace

/* sw_pack_rounds<E> on count cases of at most E·512 positions: mk[p] the round
 * mask and sto[p] the residual state (r | w << 8) of position p. */
extern "C" int pack_probe_block(int32_t E, int32_t count, const int64_t* off, const int32_t* T,
                                const int32_t* G, const int32_t* caps, const int32_t* has, const uint32_t* st,
                                uint64_t* mk, uint32_t* sto) {
    loop_kernel k = E == 2 ? k_probe_block<2> : E == 4 ? k_probe_block<4> : E == 8 ? k_probe_block<8>
                  : E == 20 ? k_probe_block<20> : E == 32 ? k_probe_block<32> : E == 64 ? k_probe_block<64>
                  : nullptr;
    if (!k) return (int)hipErrorInvalidValue;
    return run_loop(k, SW_BLOCK, (int64_t)E * SW_BLOCK, count, off, T, G, caps, has, st, mk, sto);
}

/* sw_pack_rounds_wave<E1> on count cases of at most 64·E1 positions. */
extern "C" int pack_probe_wave(int32_t E1, int32_t count, const int64_t* off, const int32_t* T,
                               const int32_t* G, const int32_t* caps, const int32_t* has, const uint32_t* st,
                               uint64_t* mk, uint32_t* sto) {
    loop_kernel k = E1 == 2 ? k_probe_wave<2> : E1 == 4 ? k_probe_wave<4> : E1 == 6 ? k_probe_wave<6>
                  : E1 == 8 ? k_probe_wave<8> : E1 == 16 ? k_probe_wave<16> : E1 == 32 ? k_probe_wave<32>
                  : E1 == 64 ? k_probe_wave<64> : nullptr;
    if (!k) return (int)hipErrorInvalidValue;
    return run_loop(k, 64, (int64_t)E1 * 64, count, off, T, G, caps, has, st, mk, sto);
}

/* sw_pack_rounds_one<multi != 0> on count cases of at most 512 positions. */
extern "C" int pack_probe_one(int32_t multi, int32_t count, const int64_t* off, const int32_t* T,
                              const int32_t* G, const int32_t* caps, const int32_t* has, const uint32_t* st,
                              uint64_t* mk, uint32_t* sto) {
    return run_loop(multi ? k_probe_one<true> : k_probe_one<false>, SW_BLOCK, SW_BLOCK, count, off, T, G, caps,
                    has, st, mk, sto);
}

/* sw_pack_room on count capacity rows: ra, rb [count][64][64] (round, lane;
 * rounds past T untouched), cb[count]. */
extern "C" int pack_probe_room(int32_t count, const int32_t* T, const int32_t* G, const int32_t* caps,
                               const int32_t* has, int32_t* ra, int32_t* rb, int32_t* cb) {
    if (count < 0) return (int)hipErrorInvalidValue;
    if (count == 0) return (int)hipSuccess;
    if (!rows_ok(count, T, G, caps, has)) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)count * 64 * 64;
    dev_pool P;
    int32_t* d_T = P.up(T, (size_t)count);
    int32_t* d_G = P.up(G, (size_t)count);
    int32_t* d_caps = P.up(caps, (size_t)count * 64);
    int32_t* d_has = P.up(has, (size_t)count);
    int32_t* d_ra = P.up(ra, n);
    int32_t* d_rb = P.up(rb, n);
    int32_t* d_cb = P.up((const int32_t*)nullptr, (size_t)count);
    if (P.err != hipSuccess) return (int)P.err;
    hipLaunchKernelGGL(k_probe_room, dim3(count), dim3(64), 0, 0, d_T, d_G, d_caps, d_has, d_ra, d_rb, d_cb);
    P.err = hipGetLastError();
    if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
    P.down(ra, d_ra, n);
    P.down(rb, d_rb, n);
    P.down(cb, d_cb, (size_t)count);
    return (int)P.err;
}

/* The wave primitives on nw pairs of 64-lane vectors (vs: sort, min, max; va:
 * the scans and the sum; wout [nw][6][64]) and the block primitives on nb
 * pairs of 512-value vectors (bout [nb][8][512]); the layouts are at the
 * kernels. */
extern "C" int pack_probe_prims(int32_t nw, const int32_t* vs, const int32_t* va, int32_t* wout, int32_t nb,
                                const int32_t* ba, const int32_t* bb, int32_t* bout) {
    if (nw < 0 || nb < 0) return (int)hipErrorInvalidValue;
    dev_pool P;
    if (nw > 0) {
        const size_t n = (size_t)nw * 64;
        int32_t* d_vs = P.up(vs, n);
        int32_t* d_va = P.up(va, n);
        int32_t* d_o = P.up((const int32_t*)nullptr, n * 6);
        if (P.err != hipSuccess) return (int)P.err;
        hipLaunchKernelGGL(k_probe_wave_prims, dim3(nw), dim3(64), 0, 0, d_vs, d_va, d_o);
        P.err = hipGetLastError();
        if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
        P.down(wout, d_o, n * 6);
    }
    if (nb > 0 && P.err == hipSuccess) {
        const size_t n = (size_t)nb * SW_BLOCK;
        int32_t* d_a = P.up(ba, n);
        int32_t* d_b = P.up(bb, n);
        int32_t* d_o = P.up((const int32_t*)nullptr, n * 8);
        if (P.err != hipSuccess) return (int)P.err;
        hipLaunchKernelGGL(k_probe_block_prims, dim3(nb), dim3(SW_BLOCK), 0, 0, d_a, d_b, d_o);
        P.err = hipGetLastError();
        if (P.err == hipSuccess) P.err = hipDeviceSynchronize();
        P.down(bout, d_o, n * 8);
    }
    return (int)P.err;
}
