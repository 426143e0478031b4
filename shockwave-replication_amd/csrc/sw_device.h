/*
 * sw_device.h — device-side batch layout shared by sw_kernels.hip and the
 * host API (sw_api.hip).
 *
 * HBM layout (structure of arrays, one batch of independent instances):
 *   per-job inputs      w[int32] d[f64] F[int32] E[int32] R[f64] p[f64]
 *                       concatenated over instances (instance i starts at
 *                       inst[i].job_off)
 *   plan bytes          [Σ_i N_i·T_i] row-major per instance ([N_i][T_i])
 *   planned rounds      [Σ_i N_i] int32
 *   round masks         [Σ_i N_i] u64 (bit t: round t), the plan kernel's
 *                       final placement, read by the P2 exchange kernel
 *   per-instance out    sw_out_dev
 *   workspace (only for instances with N > SW_LDS_JOBS): per-job state,
 *                       fp32 key rows [job][KT], masks, sort keys.
 */
#pragma once
#include <stdint.h>

#include "sw_arith.h"

#define SW_STAMP_SLOTS 64 /* per-instance u64 slots of the SW_STAMPS diagnostic build (32…42: sw_p2x_kernel, 48…52: pack sub-phases) */
#define SW_LDS_JOBS 1024 /* instances up to this many jobs keep all state on chip (2 per thread) */
/* A batch whose largest instance has maxN jobs and maxT rounds runs on chip:
 * per-job state in LDS, 32-key rows in registers; otherwise the workspace path. */
inline bool sw_on_chip(int maxN, int maxT) { return maxN <= SW_LDS_JOBS && maxT <= 32; }

struct sw_inst_dev {
    int32_t N, T, G, nb;
    int64_t job_off;
    int64_t plan_off;
    double delta, k;
    double beta[SW_BMAX];
    double ell[SW_BMAX];
};

struct sw_out_dev {
    double objective, utility, makespan, p2_objective, bound;
    int32_t iters, status;
};

/* Σ_t t·bit_t of a round mask: bit b of t weighted 2^b, six popcounts.  At
 * most 2016, summed in 32 bits: as a 64-bit value returned from a helper the
 * sum took 64-bit adds and the two-part conversion to double, and
 * sw_pack_kernel ran 0.9 % slower on the C5 sweep. */
__device__ __forceinline__ int32_t sw_mask_tsum(uint64_t m) {
    return __popcll(m & 0xAAAAAAAAAAAAAAAAull) + 2 * __popcll(m & 0xCCCCCCCCCCCCCCCCull) +
           4 * __popcll(m & 0xF0F0F0F0F0F0F0F0ull) + 8 * __popcll(m & 0xFF00FF00FF00FF00ull) +
           16 * __popcll(m & 0xFFFF0000FFFF0000ull) + 32 * __popcll(m & 0xFFFFFFFF00000000ull);
}
/* A job's term of the P2 objective: the mean round of its mask m (cnt > 0
 * rounds) weighted by its priority p. */
__device__ __forceinline__ double sw_p2_term(uint64_t m, int cnt, double p) {
    return ((double)sw_mask_tsum(m) / (double)cnt) * p;
}

/* Global workspace, per job (used only when N > SW_LDS_JOBS). */
struct sw_ws_dev {
    uint8_t* u8;    /* [total_jobs][SW_WS_U8]      */
    uint64_t* u64;  /* [total_jobs][SW_WS_U64]     */
    uint64_t* sort; /* [2·total_jobs][2] sort keys  */
    float* keys;    /* [total_jobs][KT]             */
    sw_jobc* jc;    /* [total_jobs]                 */
};
#define SW_WS_U8 8   /* per-job u8 state arrays   */
#define SW_WS_U64 6  /* per-job u64 arrays        */
/* per-instance u64 padding of the u64 workspace: the round loop's position
 * slots (pmask, pst, pord; slot = (p mod PPL)·64 + p div PPL with
 * PPL = ⌈A/64⌉) reach up to A + 62, so each slot array holds N + 64 entries */
#define SW_WS_PAD_U64 192

/* Per-instance result of the level-search kernel (sw_level_kernel), read by
 * the pack kernel (sw_pack_kernel). */
struct sw_lvl_dev {
    double U, M, bound; /* utility and makespan of the best level's counts, P1 bound */
    int64_t passes;
};
/* out.status of an instance the pack kernel left to the full plan kernel */
#define SW_STATUS_SLOW_MARK 0x40000000

struct sw_batch_dev {
    const sw_inst_dev* inst;
    int32_t count;
    int32_t KT;
    const int32_t* w;
    const double* d;
    const int32_t* F;
    const int32_t* E;
    const double* R;
    const double* p;
    uint8_t* plan;
    int32_t* planned;
    uint64_t* masks;
    sw_out_dev* out;
    uint8_t* nb;      /* level-search counts per job (sw_level_kernel → sw_pack_kernel) */
    sw_lvl_dev* lvl;  /* per instance                                              */
    int32_t only_slow; /* sw_plan_kernel: solve only instances marked SW_STATUS_SLOW_MARK */
    sw_ws_dev ws;
    unsigned char* p2ws; /* P2 exchange arrays, SW_P2X_ARR_BYTES per job (sw_p2x_inst.h) */
    int32_t fuse_p2x;    /* sw_plan_kernel: run the exchange step after the solve (sw_p2x_inst.h) */
    int32_t want_masks;  /* sw_pack_kernel: store the final masks (a caller asked for plan_masks) */
    int32_t lds_bytes;   /* sw_pack_kernel: its dynamic LDS allocation (the exchange arrays' room) */
    int32_t loop_split;  /* sw_launch_split: the pack stage as sort / rounds / place kernels (0: sw_pack_kernel) */
    /* their workspace, indexed like nb (position p of an instance at job_off + p,
     * p < A ≤ N): position words r | w << 8 | job << 16, round masks; and the
     * positions per instance (−1: marked for sw_plan_kernel) */
    uint32_t* lws;
    uint64_t* lwm;
    int32_t* lwa;
    uint64_t* stamps; /* diagnostic builds only (SW_STAMPS): [count][SW_STAMP_SLOTS] cycles (8…13: pack round-loop phases, 16…: level search, 32…: exchange) */
};
