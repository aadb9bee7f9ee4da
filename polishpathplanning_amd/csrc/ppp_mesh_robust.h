/*
 * ppp_mesh_robust.h -- robust registration of a handle's cloud, the scan, to a resident triangle mesh
 * (ppp_get_mesh_robust_registration_terms, ppp_register_mesh_robust): ppp_register_mesh's pairs and
 * residuals -- the moved point in double, the nearest indexed triangle by (D2, f), its exact closest point, the facet's own
 * normal -- under ppp_register_robust's weights: the key of (float)fabs(r), the median through ppp_trimmed.h's three digit
 * histograms at keep 0.5, sigma, Tukey's biweight, the 30 weighted words.  An evaluation pays the grid walk once: k_mesh_rob_pair
 * (the walk, a thread per query: the winning record, the residual, the key), k_mesh_rob_digit0 (the top digit's counts over the
 * stored keys; inside the walk's launch in a MESH_ROB_DIGIT_PASS=0 build), k_trim_narrow<1> and <2> as they are, k_mesh_rob_terms (tau,
 * sigma, the weighted sums over the stored winners) and k_reg_step, unchanged.  k_rob_fill stands before the chain and
 * k_rob_scatter behind it, both as ppp_robust.h has them.
 * The facet's orientation is not applied: n -> -n negates r and J together, so |r|, the key, the weight (even in r) and every
 * product are the same doubles either way, and so is every word and row.  The residual map carries r as the record's own normal
 * signs it.
 * rob_add_terms on doubles is a sibling of ppp_robust.h's float4 form, not a variant of it: k_rob_terms, k_mesh_reg_sum and the
 * walk's other callers keep their code, and with it their registers, untouched.
 */
#pragma once
#include "ppp_robust.h"
#include "ppp_mesh_registration.h"

/* 1 (the default, by measurement: DESIGN.md 7v, profiles/mesh_robust_registration_times.jsonl): k_mesh_rob_pair stores the keys
   only and k_mesh_rob_digit0, grid-stride over them under the narrow passes' grid, counts their top digits; 0: k_mesh_rob_pair
   counts them itself in an LDS histogram flushed once per workgroup, as k_rob_pair does -- a barrier behind a long, divergent
   walk and 4 000 flushes of 2 048 bins for a million queries.  The counts are integers: the same histogram either way */
#ifndef MESH_ROB_DIGIT_PASS
#define MESH_ROB_DIGIT_PASS 1
#endif
/* the workgroups of k_mesh_rob_terms are capped at MESH_ROB_GRID_CUS per compute unit, as k_mesh_reg_sum's are (0: no cap);
   integer sums make the words independent of it: measured over 2, 4, 8 and none, 2 was the fastest */
#ifndef MESH_ROB_GRID_CUS
#define MESH_ROB_GRID_CUS 2
#endif

/* B.104's terms for a normal that is three doubles already (the facet's own): ppp_robust.h's float4 form, operation for
   operation, without its widening casts; u and J are icp_add_terms's on doubles.  With w = 1 every word is that function's. */
__device__ __attribute__((always_inline)) inline void rob_add_terms(unsigned long long *a, const double *m, double r, double w, const double *n,
                                                                   const IcpFrame &F)
{
    const double nx = n[0], ny = n[1], nz = n[2];
    const double ux = (m[0] - F.c[0]) / F.Ln, uy = (m[1] - F.c[1]) / F.Ln, uz = (m[2] - F.c[2]) / F.Ln;
    const double J[6] = {uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx, nx, ny, nz};
    if (w > 0.0) a[ROB_USED] += 1;
    int at = ICP_A;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int k = i; k < 6; ++k, ++at) a[at] += (unsigned long long)llrint(((J[i] * J[k]) * w) * F.scale);
        a[ICP_B + i] += (unsigned long long)llrint(((J[i] * r) * w) * F.scale);
    }
    a[ICP_E] += (unsigned long long)llrint(((r * r) * w) * F.scale);
    a[ROB_WSUM] += (unsigned long long)llrint(w * F.scale);
}

/* B.131: k_mesh_reg_search's walk, a thread per indexed point of the scan in slab order (q4 = its sorted4, nq = its n_sorted;
   TM_T == TRIM_T).  A pair (B.r >= 0 and D2 <= md2, inclusive) leaves the winning record's number, the residual of the moved
   point against the exact closest point along the record's own normal -- k_mesh_reg_sum's e, n and r, on the walk's x -- and the
   key of (float)fabs(r); any other query the key TRIM_NONE.  No sums here: the walk's doubles beside the accumulators are what
   brought k_mesh_reg_terms to one wave a SIMD. */
__global__ void __launch_bounds__(TM_T) k_mesh_rob_pair(const float4 *__restrict__ q4, int nq, const TriGrid G, double md2, const double *__restrict__ T,
        const IcpCtl *__restrict__ ctl, unsigned *__restrict__ win, double *__restrict__ res, u32 *__restrict__ key, u32 *__restrict__ hist0)
{
    if (ctl->done) return;
#if !MESH_ROB_DIGIT_PASS
    static_assert(TM_T == TRIM_T, "trim_flush strides by TRIM_T");
    __shared__ u32 s_h[TRIM_B0];
    for (int b = threadIdx.x; b < TRIM_B0; b += TM_T) s_h[b] = 0;
    __syncthreads();
#endif
    const int at = blockIdx.x * TM_T + threadIdx.x;
    if (at < nq) {
        double t[12], m[3];
#pragma unroll
        for (int i = 0; i < 12; ++i) t[i] = T[i];
        icp_move(t, q4[at], m);
        u32 kk = TRIM_NONE;
        if (isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2])) {
            TmBest B;
            tm_nearest(G, m, md2, B);
            if (B.r >= 0 && B.D2 <= md2) {
                double p0[3], p1[3], p2[3], N[3];
                int f;
                tm_load(G.rec, B.r, p0, p1, p2, &f);
                const double A2 = tm_normal(p0, p1, p2, N);
                const double ex = m[0] - B.x[0], ey = m[1] - B.x[1], ez = m[2] - B.x[2];
                const double r = ((ex * (N[0] / A2)) + ey * (N[1] / A2)) + ez * (N[2] / A2);
                kk = __float_as_uint((float)fabs(r));
                win[at] = (unsigned)B.r;
                res[at] = r;
#if !MESH_ROB_DIGIT_PASS
                atomicAdd(&s_h[kk >> 21], 1u);
#endif
            }
        }
        key[at] = kk;
    }
#if !MESH_ROB_DIGIT_PASS
    __syncthreads();
    trim_flush(s_h, TRIM_B0, hist0);
#endif
}

/* the top digits of the stored keys, where k_mesh_rob_pair does not count them (MESH_ROB_DIGIT_PASS): grid-stride, an LDS
   histogram per workgroup, one flush */
__global__ void __launch_bounds__(TRIM_T) k_mesh_rob_digit0(const u32 *__restrict__ key, int nq, const IcpCtl *__restrict__ ctl, u32 *__restrict__ hist0)
{
    if (ctl->done) return;
    __shared__ u32 s_h[TRIM_B0];
    for (int b = threadIdx.x; b < TRIM_B0; b += TRIM_T) s_h[b] = 0;
    __syncthreads();
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        const u32 kk = key[at];
        if (kk != TRIM_NONE) atomicAdd(&s_h[kk >> 21], 1u);
    }
    __syncthreads();
    trim_flush(s_h, TRIM_B0, hist0);
}

/* B.133: k_rob_terms's prologue -- tau from hist (k_trim_narrow<2>'s counts) at the rank it left, sigma, cs; workgroup 0 leaves
   tau and sigma for the host and the scatter -- then the 30 weighted words over the paired queries, grid-stride: the point moved
   again from T (icp_move), the stored record loaded and its normal made again (tm_load, tm_normal, N / A2: k_mesh_reg_sum's
   operations on the same operands), the residual read back -- the closest point enters nothing else, so it is not made again --,
   rob_weight, rob_add_terms on doubles, rob_flush. */
__global__ void __launch_bounds__(TRIM_T) k_mesh_rob_terms(const float4 *__restrict__ q4, int nq, const TriGrid G, const IcpFrame F, const RobScale S,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, const unsigned *__restrict__ win, const double *__restrict__ res,
        const u32 *__restrict__ key, const u32 *hist, TrimCut *cut, double *sigma_out, unsigned long long *__restrict__ acc)
{
    if (ctl->done) return;
    __shared__ unsigned long long s_a[TRIM_T / 64][ROB_WORDS];
    __shared__ int s_scr[16];
    __shared__ u32 s_out[4];
    if (cut->paired == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { cut->tau = TRIM_NAN; *sigma_out = icp_nan(); }
        return;
    }
    trim_select<TRIM_B2 / TRIM_T>(hist, false, 0.0, cut->rank2, s_scr, s_out);
    const u32 tau = cut->prefix2 | s_out[0];
    const double sigma = rob_sigma(tau, false, S.sigma_min);
    const double cs = S.tune * sigma;
    if (blockIdx.x == 0 && threadIdx.x == 0) { cut->tau = tau; *sigma_out = sigma; }
    unsigned long long a[ROB_WORDS];
#pragma unroll
    for (int w = 0; w < ROB_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        if (key[at] == TRIM_NONE) continue;
        const unsigned rec = win[at];
        if (rec >= (unsigned)G.indexed) continue; /* (never: a key that is not TRIM_NONE has its record beside it) */
        double m[3], p0[3], p1[3], p2[3], N[3];
        int f;
        icp_move(t, q4[at], m);
        tm_load(G.rec, (int)rec, p0, p1, p2, &f);
        const double A2 = tm_normal(p0, p1, p2, N);
        const double n[3] = {N[0] / A2, N[1] / A2, N[2] / A2};
        const double r = res[at];
        rob_add_terms(a, m, r, rob_weight(r, cs, S.tune), n, F);
    }
    rob_flush(a, s_a, acc);
}
