/*
 * oracle/p2x_twin.c — TEST INFRASTRUCTURE, NOT PRODUCT CODE.
 *
 * Sequential specification of the P2 exchange step (negative-cycle
 * cancelling over round moves, csrc/sw_p2x.h) that the GPU
 * kernel (csrc/sw_p2x_kernel.hip) and the sharded engine run in parallel.
 * The plan twin (plan_twin.c) calls it on its final P2 placement and the CPU
 * shard engine (shard_twin.c) on the gathered placement; the GPU must return
 * the same masks bit for bit.  Reference: the P2 MILP, shockwave.py:281-328.
 *
 * Layout.  Active jobs (n_j > 0) are grouped by width class (classes in
 * ascending width), and inside a class ranked by (c desc, job asc) with
 * c = p/n.  Position p = off[k] + rank.  Class k's membership of round t is
 * a bitset over its ranks, nw[k] words at B + boff[k] + t·nw[k].
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/shockwave_amd.h"
#include "../shockwave-replication_amd/csrc/sw_p2x.h"

double twin_detsum(const double* v, int32_t N); /* plan_twin.c */

typedef struct {
    int32_t job;
    double c;
} p2x_ent;

/* (sw_p2x_ckey(c) desc, job asc) */
static int ent_cmp(const void* a, const void* b) {
    const p2x_ent* x = (const p2x_ent*)a;
    const p2x_ent* y = (const p2x_ent*)b;
    const uint64_t kx = sw_p2x_ckey(x->c), ky = sw_p2x_ckey(y->c);
    if (kx != ky) return kx > ky ? -1 : 1;
    return x->job < y->job ? -1 : (x->job > y->job);
}

typedef struct {
    int32_t T, G, K, A;
    int32_t wc[SW_P2X_KMAX], M[SW_P2X_KMAX], off[SW_P2X_KMAX], nw[SW_P2X_KMAX], boff[SW_P2X_KMAX];
    int32_t* pjob;  /* [A] job of position p          */
    double* pc;     /* [A] c of position p            */
    uint64_t* pm;   /* [A] round mask of position p   */
    uint64_t* B;    /* class × round rank bitsets     */
    int32_t room[SW_TMAX];
    double W[SW_TMAX * SW_TMAX]; /* W[t·T + u], δ included; SW_P2X_NONE = no edge */
    int8_t Wk[SW_TMAX * SW_TMAX]; /* class of the edge                         */
} p2x_t;

static uint64_t* bits(p2x_t* X, int32_t k, int32_t t) { return X->B + X->boff[k] + (size_t)t * X->nw[k]; }

/* W for load size F: per edge the cheapest class (ascending class on ties). */
static void build_w(p2x_t* X, int32_t F, double delta) {
    const int32_t T = X->T;
    for (int32_t t = 0; t < T; ++t) {
        for (int32_t u = 0; u < T; ++u) {
            double best = SW_P2X_NONE;
            int32_t bk = -1;
            if (u != t) {
                for (int32_t k = 0; k < X->K; ++k) {
                    if (X->wc[k] > F || F % X->wc[k] != 0 || F / X->wc[k] > SW_P2X_QMAX) continue;
                    const double cost = sw_p2x_cost(bits(X, k, t), bits(X, k, u), X->nw[k], 1, F / X->wc[k],
                                                    t, u, X->pc + X->off[k]);
                    if (cost < best) { best = cost; bk = k; }
                }
            }
            X->W[t * T + u] = bk >= 0 ? best + delta : SW_P2X_NONE;
            X->Wk[t * T + u] = (int8_t)bk;
        }
    }
}

/* Bellman–Ford (Jacobi) over rounds 0..T−1 and V = T; after the odd
 * sweeps and the last the predecessor graph is checked for a cycle (the one reached from the
 * lowest round whose predecessor walk never ends).  Returns its length and
 * its nodes from the lowest one in predecessor order (cyc[i+1] =
 * pred(cyc[i])) when its cost is negative, else 0.
 *
 * Warm start: dw holds the distances this load size's previous run ended
 * with; when warm, the sweeps start from them instead of 0 (any start gives
 * the same verdict on a graph without a negative cycle — no change within
 * T + 1 sweeps means the distances are feasible potentials — and a cycle of
 * the predecessor graph is negative from any start), and the predecessor
 * graph is also checked after the first sweep.  The run leaves its last
 * distances in dw.  Most runs follow a cancel that changed a few rows and
 * columns of W, where the old potentials are nearly feasible: C3 instances
 * take 31 instead of 42 sweeps, the C5 mix 54 instead of 97. */
static int32_t find_cycle(const p2x_t* X, int32_t F, int32_t* cyc, double* dw, int warm) {
    const int32_t T = X->T;
    double d[SW_TMAX + 1], nd[SW_TMAX + 1];
    int32_t pr[SW_TMAX + 1], np[SW_TMAX + 1];
    for (int32_t x = 0; x <= T; ++x) { d[x] = warm ? dw[x] : 0.0; pr[x] = -1; }
    for (int32_t it = 0; it <= T; ++it) {
        int changed = 0;
        for (int32_t u = 0; u < T; ++u) {
            double best = d[u];
            int32_t bp = pr[u];
            for (int32_t t = 0; t < T; ++t) {
                const double w = X->W[t * T + u];
                if (t == u || !(w < SW_P2X_NONE)) continue;
                const double v = d[t] + w;
                if (v < best) { best = v; bp = t; }
            }
            if (d[T] < best) { best = d[T]; bp = T; } /* V → u, cost 0 */
            nd[u] = best;
            np[u] = bp;
            changed |= best < d[u];
        }
        {
            double best = d[T];
            int32_t bp = pr[T];
            for (int32_t t = 0; t < T; ++t)
                if (X->room[t] >= F && d[t] < best) { best = d[t]; bp = t; } /* t → V, cost 0 */
            nd[T] = best;
            np[T] = bp;
            changed |= best < d[T];
        }
        if (!changed) {
            for (int32_t x = 0; x <= T; ++x) dw[x] = d[x];
            return 0;
        }
        for (int32_t x = 0; x <= T; ++x) { d[x] = nd[x]; pr[x] = np[x]; dw[x] = d[x]; }
        /* checked after the odd sweeps and the last one (from d = 0, after
         * the first sweep every predecessor is a later round: no cycle can
         * exist yet; from warm distances also after the first) */
        if (!(it & 1) && it != T && !(warm && it == 0)) continue;
        /* a cycle of the predecessor graph: T + 1 steps from x still defined */
        for (int32_t x = 0; x <= T; ++x) {
            int32_t y = x;
            for (int32_t s = 0; s <= T && y >= 0; ++s) y = pr[y];
            if (y < 0) continue;
            /* the cycle from its lowest node */
            int32_t lo = y;
            for (int32_t v = pr[y]; v != y; v = pr[v]) lo = v < lo ? v : lo;
            int32_t len = 0, v = lo;
            do { cyc[len++] = v; v = pr[v]; } while (v != lo);
            /* its exact cost, in this order (edges pred(v) → v) */
            double cost = 0.0;
            for (int32_t i = 0; i < len; ++i) {
                const int32_t u = cyc[i], t = pr[u];
                if (u < T && t < T) cost = cost + X->W[t * T + u];
            }
            return cost < 0.0 ? len : 0;
        }
    }
    return 0;
}

/* Moves the selections of every edge of the cycle (all selected first, from
 * the state before the cycle, then applied). */
static void cancel(p2x_t* X, int32_t F, const int32_t* cyc, int32_t len, int32_t* tmp) {
    const int32_t T = X->T;
    int32_t nsel = 0;
    for (int32_t i = 0; i < len; ++i) {
        const int32_t u = cyc[i], t = cyc[(i + 1) % len]; /* pred(u) = t */
        if (u == T || t == T) continue;
        const int32_t k = X->Wk[t * T + u];
        const int32_t q = F / X->wc[k];
        int32_t r = sw_p2x_start(bits(X, k, t), bits(X, k, u), X->nw[k], 1, q, u < t);
        for (int32_t g = 0; g < q; ++g) {
            tmp[nsel++] = (k << 24) | (t << 16) | (u << 8);
            tmp[nsel++] = r;
            if (g + 1 < q) r = sw_p2x_next(bits(X, k, t), bits(X, k, u), X->nw[k], 1, r + 1);
        }
    }
    for (int32_t i = 0; i < nsel; i += 2) {
        const int32_t k = tmp[i] >> 24, t = (tmp[i] >> 16) & 0xFF, u = (tmp[i] >> 8) & 0xFF;
        const int32_t r = tmp[i + 1];
        bits(X, k, t)[r >> 6] &= ~(1ull << (r & 63));
        bits(X, k, u)[r >> 6] |= 1ull << (r & 63);
        X->pm[X->off[k] + r] ^= (1ull << t) | (1ull << u);
        X->room[t] += X->wc[k];
        X->room[u] -= X->wc[k];
    }
}

/* The step's set-up: classes, positions, rank bitsets, free capacity and δ.
 * NULL when the step is skipped (no jobs, T < 2, more than SW_P2X_AMAX jobs
 * or more than SW_P2X_KMAX width classes). */
static p2x_t* p2x_open(int32_t A, int32_t T, int32_t G, const int32_t* job, const int32_t* w,
                       const double* c, const uint64_t* m, double* delta) {
    if (A <= 0 || T < 2 || A > SW_P2X_AMAX) return NULL;
    p2x_t* X = (p2x_t*)calloc(1, sizeof(p2x_t));
    X->T = T;
    X->G = G;
    for (int32_t i = 0; i < A; ++i) {
        int32_t k = 0;
        while (k < X->K && X->wc[k] != w[i]) ++k;
        if (k == X->K) {
            if (X->K == SW_P2X_KMAX) { free(X); return NULL; }
            X->wc[X->K++] = w[i];
        }
    }
    /* classes ascending */
    for (int32_t a = 1; a < X->K; ++a)
        for (int32_t b = a; b > 0 && X->wc[b - 1] > X->wc[b]; --b) {
            const int32_t s = X->wc[b]; X->wc[b] = X->wc[b - 1]; X->wc[b - 1] = s;
        }
    X->A = A;
    X->pjob = (int32_t*)malloc(sizeof(int32_t) * A);
    X->pc = (double*)malloc(sizeof(double) * A);
    X->pm = (uint64_t*)malloc(sizeof(uint64_t) * A);
    p2x_ent* e = (p2x_ent*)malloc(sizeof(p2x_ent) * A);
    int32_t p = 0, nb = 0;
    for (int32_t k = 0; k < X->K; ++k) {
        int32_t M = 0;
        for (int32_t i = 0; i < A; ++i)
            if (w[i] == X->wc[k]) { e[M].job = job[i]; e[M].c = c[i]; ++M; }
        qsort(e, (size_t)M, sizeof(p2x_ent), ent_cmp);
        X->M[k] = M;
        X->off[k] = p;
        X->nw[k] = (M + 63) / 64;
        X->boff[k] = nb;
        nb += X->nw[k] * T;
        for (int32_t r = 0; r < M; ++r) {
            X->pjob[p + r] = e[r].job;
            X->pc[p + r] = e[r].c;
        }
        p += M;
    }
    /* masks by position (the job ids are unique) */
    for (int32_t q = 0; q < A; ++q) {
        int32_t lo = 0, hi = A - 1; /* job is ascending in the input */
        const int32_t jq = X->pjob[q];
        while (lo < hi) {
            const int32_t mid = (lo + hi) / 2;
            if (job[mid] < jq) lo = mid + 1; else hi = mid;
        }
        X->pm[q] = m[lo];
    }
    X->B = (uint64_t*)calloc((size_t)(nb > 0 ? nb : 1), sizeof(uint64_t));
    for (int32_t t = 0; t < T; ++t) X->room[t] = G;
    double* v = (double*)malloc(sizeof(double) * A);
    for (int32_t k = 0; k < X->K; ++k)
        for (int32_t r = 0; r < X->M[k]; ++r) {
            const int32_t q = X->off[k] + r;
            int64_t S = 0;
            for (int32_t t = 0; t < T; ++t)
                if ((X->pm[q] >> t) & 1ull) {
                    bits(X, k, t)[r >> 6] |= 1ull << (r & 63);
                    X->room[t] -= X->wc[k];
                    S += t;
                }
            v[q] = X->pc[q] * (double)S;
        }
    *delta = sw_p2x_delta(twin_detsum(v, A), T, A);
    free(v); free(e);
    return X;
}

static void p2x_close(p2x_t* X) {
    free(X->pjob); free(X->pc); free(X->pm); free(X->B); free(X);
}

/*
 * The exchange step on the active jobs (ascending job order): job[i], w[i],
 * c[i] = p/n, m[i] (round mask, improved in place).  Returns the number of
 * cycles cancelled; 0 (no change) when there are more than SW_P2X_KMAX
 * width classes.
 */
int32_t twin_p2x_run(int32_t A, int32_t T, int32_t G, const int32_t* job, const int32_t* w,
                     const double* c, uint64_t* m) {
    double delta;
    p2x_t* X = p2x_open(A, T, G, job, w, c, m, &delta);
    if (!X) return 0;
    int32_t cyc[SW_TMAX + 1];
    int32_t* tmp = (int32_t*)malloc(sizeof(int32_t) * 2 * (size_t)SW_P2X_MAX_MOVES);
    int32_t ncancel = 0;
    double dw[SW_P2X_KMAX][SW_TMAX + 1]; /* each load size's last distances */
    int have[SW_P2X_KMAX] = {0};
    /* cert[k]: the cancel count when load size k last found no cycle; while
     * nothing was cancelled since, its graph is unchanged and the repeat pass
     * skips it (a warm rerun could continue a descent the last run stopped
     * at its sweep limit, so the skip is part of the specification) */
    int32_t cert[SW_P2X_KMAX];
    for (int32_t k = 0; k < SW_P2X_KMAX; ++k) cert[k] = -1;
    for (int changed = 1; changed && ncancel < SW_P2X_MAX_CANCEL;) {
        changed = 0;
        for (int32_t ki = 0; ki < X->K && ncancel < SW_P2X_MAX_CANCEL; ++ki) {
            const int32_t F = X->wc[ki];
            if (cert[ki] == ncancel) continue;
            while (ncancel < SW_P2X_MAX_CANCEL) {
                build_w(X, F, delta);
                const int32_t len = find_cycle(X, F, cyc, dw[ki], have[ki]);
                have[ki] = 1;
                if (len == 0) {
                    cert[ki] = ncancel;
                    break;
                }
                int32_t moves = 0; /* the cycle's job moves */
                for (int32_t i = 0; i < len; ++i) {
                    const int32_t u = cyc[i], t = cyc[(i + 1) % len];
                    if (u < T && t < T) moves += F / X->wc[X->Wk[t * T + u]];
                }
                if (moves > SW_P2X_MAX_MOVES) break;
                cancel(X, F, cyc, len, tmp);
                ++ncancel;
                changed = 1;
            }
        }
    }
    /* back to the input order */
    for (int32_t q = 0; q < A; ++q) {
        int32_t lo = 0, hi = A - 1;
        const int32_t jq = X->pjob[q];
        while (lo < hi) {
            const int32_t mid = (lo + hi) / 2;
            if (job[mid] < jq) lo = mid + 1; else hi = mid;
        }
        m[lo] = X->pm[q];
    }
    free(tmp);
    p2x_close(X);
    return ncancel;
}

/* ---- entry points for the step's own tests (tests/test_p2x.py) ---- */

/* find_cycle on a given graph: W[T·T] (δ included, SW_P2X_NONE = no edge),
 * room[T] against load size F, dw[T + 1] the warm distances in and the last
 * distances out.  Returns the cycle's length, its nodes in cyc[T + 1]. */
int32_t twin_p2x_find_cycle(int32_t T, int32_t F, const double* W, const int32_t* room, double* dw,
                            int32_t warm, int32_t* cyc) {
    if (T < 2 || T > SW_TMAX) return -1;
    p2x_t* X = (p2x_t*)calloc(1, sizeof(p2x_t));
    X->T = T;
    memcpy(X->W, W, sizeof(double) * (size_t)T * T);
    memcpy(X->room, room, sizeof(int32_t) * (size_t)T);
    const int32_t len = find_cycle(X, F, cyc, dw, warm != 0);
    free(X);
    return len;
}

/* The set-up of twin_p2x_run on a placement and one build_w for load size F:
 * W[T·T] (δ included) and Wk[T·T] out.  Returns δ; -1 when the step is
 * skipped (W, Wk untouched). */
double twin_p2x_edges(int32_t A, int32_t T, int32_t G, const int32_t* job, const int32_t* w,
                      const double* c, const uint64_t* m, int32_t F, double* W, int8_t* Wk) {
    double delta;
    p2x_t* X = p2x_open(A, T, G, job, w, c, m, &delta);
    if (!X) return -1.0;
    build_w(X, F, delta);
    memcpy(W, X->W, sizeof(double) * (size_t)T * T);
    memcpy(Wk, X->Wk, (size_t)T * T);
    p2x_close(X);
    return delta;
}

/* The step on a full plan (y: [N][T] bytes, counts n): used by the plan twin. */
int32_t twin_p2x_plan(int32_t N, int32_t T, int32_t G, const int32_t* w, const double* prio,
                      const int32_t* n, uint8_t* y) {
    int32_t A = 0;
    for (int32_t j = 0; j < N; ++j) A += n[j] > 0;
    if (A == 0) return 0;
    int32_t* job = (int32_t*)malloc(sizeof(int32_t) * A);
    int32_t* wa = (int32_t*)malloc(sizeof(int32_t) * A);
    double* c = (double*)malloc(sizeof(double) * A);
    uint64_t* m = (uint64_t*)malloc(sizeof(uint64_t) * A);
    int32_t i = 0;
    for (int32_t j = 0; j < N; ++j) {
        if (n[j] <= 0) continue;
        uint64_t mk = 0;
        for (int32_t t = 0; t < T; ++t) mk |= (uint64_t)(y[(size_t)j * T + t] != 0) << t;
        job[i] = j; wa[i] = w[j]; c[i] = prio[j] / (double)n[j]; m[i] = mk;
        ++i;
    }
    const int32_t nc = twin_p2x_run(A, T, G, job, wa, c, m);
    for (i = 0; i < A; ++i)
        for (int32_t t = 0; t < T; ++t) y[(size_t)job[i] * T + t] = (uint8_t)((m[i] >> t) & 1ull);
    free(job); free(wa); free(c); free(m);
    return nc;
}
