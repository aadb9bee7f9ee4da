/*
 * ppp_mesh_registration.h -- point-to-plane ICP of a handle's cloud, the scan, to a resident triangle mesh
 * (ppp_get_mesh_registration_terms, ppp_register_mesh).  An evaluation: the scan's points, moved by the current
 * transform in double (icp_move), through the mesh's grid (tm_nearest: the nearest indexed triangle by (D2, f), the exact closest
 * point), the winning facet's own normal (tm_load, tm_normal), and the 29 integer sums of the normal equations (icp_add_terms on
 * doubles) -- as two launches, k_mesh_reg_search and k_mesh_reg_sum, or as the fused k_mesh_reg_terms (MESH_REG_SPLIT).  The step
 * is k_reg_step, unchanged; the host's chain has registration_chain's shape.  Nothing here estimates a normal or knows a pitch:
 * the fit is taken on the facets that ppp_get_mesh_deviation measures against.
 * Robust weights on these pairs are ppp_mesh_robust.h's, trimmed weights and border rejection
 * ppp_mesh_trimmed.h's; the plain evaluation and loop over slice-range tiles are ppp_mesh_tile.h's;
 * the robust and trimmed loops over tiles and pseudonormals are not offered.
 * The global start from the mesh (ppp_trimesh_get_moments, ppp_register_mesh_global): k_mesh_moments, the ten
 * integer words of the surface's area moments, and mesh_frame_from_words, the frame they imply; k_mesh_reg_search_multi and
 * k_mesh_reg_sum_multi, K chains side by side on the queries StrideSel compacts once, with k_reg_step_multi for the steps.
 * The facet's orientation is not applied: n -> -n flips J and r together, so every product J_i J_k, J_i r, r r is the same
 * double either way, and so is every word.
 */
#pragma once
#include "ppp_registration.h"
#include "ppp_trimesh.h"

/* 1 (the default, by measurement: DESIGN.md 7u, profiles/mesh_registration_times.jsonl): an evaluation is k_mesh_reg_search and
   k_mesh_reg_sum (below); 0: the fused k_mesh_reg_terms, kept for the tuning build that measures one against the other */
#ifndef MESH_REG_SPLIT
#define MESH_REG_SPLIT 1
#endif
/* the workgroups of the summing kernel (k_mesh_reg_sum, or the fused k_mesh_reg_terms) are capped at MESH_REG_GRID_CUS per compute
   unit, as k_reg_terms's are (0: no cap); integer sums make the words independent of it: measured too, 2 was the fastest */
#ifndef MESH_REG_GRID_CUS
#define MESH_REG_GRID_CUS 2
#endif

/* One evaluation at T into acc: a thread per indexed point of the scan in its slab order (q4 = its sorted4, nq = its n_sorted),
   grid-stride.  The query is the moved point itself, in double; a moved point that is not finite makes no pair; a pair holds
   with D2 <= md2 (inclusive: ppp_get_mesh_deviation's bound), in every region.  T is read from device memory: the step kernel
   before this launch wrote it. */
__global__ void __launch_bounds__(ICP_T) k_mesh_reg_terms(const float4 *__restrict__ q4, int nq, const TriGrid G, const IcpFrame F, double md2,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, unsigned long long *__restrict__ acc)
{
    if (ctl->done) return;
    __shared__ unsigned long long s_a[ICP_T / 64][ICP_WORDS];
    unsigned long long a[ICP_WORDS];
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = blockIdx.x * ICP_T + threadIdx.x; at < nq; at += gridDim.x * ICP_T) {
        double m[3];
        icp_move(t, q4[at], m);
        if (!(isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2]))) continue;
        TmBest B;
        tm_nearest(G, m, md2, B);
        if (!(B.r >= 0 && B.D2 <= md2)) continue;
        double p0[3], p1[3], p2[3], N[3];
        int f;
        tm_load(G.rec, B.r, p0, p1, p2, &f);
        const double A2 = tm_normal(p0, p1, p2, N);
        const double n[3] = {N[0] / A2, N[1] / A2, N[2] / A2};
        icp_add_terms(a, m, B.x, n, F);
    }
    icp_flush<ICP_T>(a, s_a, acc);
}

/* The same evaluation as two launches (MESH_REG_SPLIT): the fused kernel holds the walk's doubles beside 58
   accumulator registers and comes to one wave a SIMD.  k_mesh_reg_search is the walk alone, a thread per query as k_mesh_nearest
   runs it: win[at] = the winning record's number, MESH_REG_NONE without a pair.  k_mesh_reg_sum moves the point again,
   recomputes tm_closest on that one record -- the same operations on the same operands: x and D2 are the walk's bits -- and sums,
   grid-stride.  The rows are the same bits either way. */
#define MESH_REG_NONE 0xffffffffu

/* k_mesh_reg_search's body for query `at`, k_mesh_reg_sum's for workgroup `block` of `blocks`: one chain's evaluation at T.  The
   single chain's kernels and the side-by-side ones call them, so a row is the same bits from either (reg_terms_body's way).
   TILE (k_mesht_reg_search, k_mesht_reg_sum; ppp_mesh_tile.h): the queries are the positions [pos0, nq) of the
   index, win[at - pos0] is a position's word, and a position whose resident, unmoved x `own` does not own (B.36) writes
   MESH_REG_NONE and counts nowhere; *mine takes the thread's count of owned positions.  The whole-cloud kernels pass pos0 = 0 and
   compile no test. */
template <bool TILE>
__device__ __forceinline__ void mesh_reg_search_body(const float4 *__restrict__ q4, int pos0, int nq, const TileRange &own, const TriGrid &G, double md2,
        const double *__restrict__ T, unsigned *__restrict__ win, int at)
{
    if (at >= nq) return;
    const float4 q = q4[at];
    unsigned w = MESH_REG_NONE;
    if (!TILE || own.owned(q.x)) {
        double t[12], m[3];
#pragma unroll
        for (int i = 0; i < 12; ++i) t[i] = T[i];
        icp_move(t, q, m);
        if (isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2])) {
            TmBest B;
            tm_nearest(G, m, md2, B);
            if (B.r >= 0 && B.D2 <= md2) w = (unsigned)B.r;
        }
    }
    win[at - pos0] = w;
}

template <bool TILE>
__device__ __forceinline__ void mesh_reg_sum_body(const float4 *__restrict__ q4, int pos0, int nq, const TileRange &own, const TriGrid &G, const IcpFrame &F,
        const double *__restrict__ T, const unsigned *__restrict__ win, unsigned long long *__restrict__ acc, int block, int blocks,
        unsigned long long *mine)
{
    __shared__ unsigned long long s_a[ICP_T / 64][ICP_WORDS];
    unsigned long long a[ICP_WORDS];
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = pos0 + block * ICP_T + threadIdx.x; at < nq; at += blocks * ICP_T) {
        if (TILE) *mine += own.owned(q4[at].x);
        const unsigned r = win[at - pos0];
        if (r >= (unsigned)G.indexed) continue; /* (MESH_REG_NONE too) */
        double m[3], p0[3], p1[3], p2[3], N[3], x[3], D2;
        int f;
        icp_move(t, q4[at], m);
        tm_load(G.rec, (int)r, p0, p1, p2, &f);
        (void)tm_closest(m, p0, p1, p2, x, &D2);
        const double A2 = tm_normal(p0, p1, p2, N);
        const double n[3] = {N[0] / A2, N[1] / A2, N[2] / A2};
        icp_add_terms(a, m, x, n, F);
    }
    icp_flush<ICP_T>(a, s_a, acc);
}

/* what the whole-cloud kernels hand the bodies for `own`: everything (never read: TILE is false) */
__device__ __forceinline__ TileRange mesh_reg_whole() { return TileRange{-INFINITY, INFINITY, -INFINITY, INFINITY}; }

__global__ void __launch_bounds__(TM_T) k_mesh_reg_search(const float4 *__restrict__ q4, int nq, const TriGrid G, double md2, const double *__restrict__ T,
        const IcpCtl *__restrict__ ctl, unsigned *__restrict__ win)
{
    if (ctl->done) return;
    mesh_reg_search_body<false>(q4, 0, nq, mesh_reg_whole(), G, md2, T, win, blockIdx.x * TM_T + threadIdx.x);
}

__global__ void __launch_bounds__(ICP_T) k_mesh_reg_sum(const float4 *__restrict__ q4, int nq, const TriGrid G, const IcpFrame F, const double *__restrict__ T,
        const IcpCtl *__restrict__ ctl, const unsigned *__restrict__ win, unsigned long long *__restrict__ acc)
{
    if (ctl->done) return;
    mesh_reg_sum_body<false>(q4, 0, nq, mesh_reg_whole(), G, F, T, win, acc, blockIdx.x, gridDim.x, nullptr);
}

/* K chains side by side (ppp_register_mesh_global): start blockIdx.y evaluates at its own transform -- T, ctl and
   acc are those of start 0, a start's lie tstride doubles, one IcpCtl and astride words behind its predecessor's
   (k_reg_terms_multi's layout), its winning records nq words behind its predecessor's.  The search is a thread per compacted
   query, uncapped as the single chain's; the sum strides with gridDim.x workgroups per start.  A chain that has ended returns at
   its first instruction, whatever the others do. */
__global__ void __launch_bounds__(TM_T) k_mesh_reg_search_multi(const float4 *__restrict__ q4, int nq, const TriGrid G, double md2, const double *__restrict__ T,
        size_t tstride, const IcpCtl *__restrict__ ctl, unsigned *__restrict__ win)
{
    if (ctl[blockIdx.y].done) return;
    mesh_reg_search_body<false>(q4, 0, nq, mesh_reg_whole(), G, md2, T + blockIdx.y * tstride, win + (size_t)blockIdx.y * (size_t)nq, blockIdx.x * TM_T + threadIdx.x);
}

__global__ void __launch_bounds__(ICP_T) k_mesh_reg_sum_multi(const float4 *__restrict__ q4, int nq, const TriGrid G, const IcpFrame F, const double *__restrict__ T,
        size_t tstride, const IcpCtl *__restrict__ ctl, const unsigned *__restrict__ win, unsigned long long *__restrict__ acc, size_t astride)
{
    if (ctl[blockIdx.y].done) return;
    mesh_reg_sum_body<false>(q4, 0, nq, mesh_reg_whole(), G, F, T + blockIdx.y * tstride, win + (size_t)blockIdx.y * (size_t)nq, acc + blockIdx.y * astride, blockIdx.x,
                             gridDim.x, nullptr);
}

/* ---------------------------------------------------------------------------------------------------------------------- */
/* The principal frame of the mesh's surface (ppp_trimesh_get_moments)                        */
/* ---------------------------------------------------------------------------------------------------------------------- */

/* min(40, 54 - clog2(max(2, n_tris))), n_tris the caller's triangle count: a term stays below 2^6 2^ms (a <= 2 sqrt 3, |q| <= 12) */
__host__ __device__ inline int mesh_mom_shift(size_t n_tris)
{
    const int s = 54 - icp_clog2((double)(n_tris < 2 ? (size_t)2 : n_tris));
    return s < 40 ? s : 40;
}

/* A thread per record, grid-stride: the corners u_i = (p_i - c) / L of tm_load's doubles, N = (u1 - u0) x (u2 - u0) and |N| by
   tm_normal, the area a = |N| 0.5, s = (u0 + u1) + u2, q_dk = ((u0_d u0_k + u1_d u1_k) + u2_d u2_k) + s_d s_k; the ten words
   llrint(a 2^ms), llrint((a s_d) 2^ms), llrint((a q_dk) 2^ms) (F.scale = 2^ms) into the thread's 64-bit integers and through
   mom_flush: k_cloud_moments's pattern.  Over a triangle the integral of u is a s / 3 and that of u_d u_k is a q_dk / 12,
   exactly: the frame weighs the surface, not the vertices. */
__global__ void __launch_bounds__(MOM_T) k_mesh_moments(const TriGrid G, const MomFrame F, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[MOM_T / 64][MOM_WORDS];
    unsigned long long a[MOM_WORDS];
#pragma unroll
    for (int w = 0; w < MOM_WORDS; ++w) a[w] = 0;
    for (int r = blockIdx.x * MOM_T + threadIdx.x; r < G.indexed; r += gridDim.x * MOM_T) {
        double p[3][3], u[3][3], N[3], s[3];
        int f;
        tm_load(G.rec, r, p[0], p[1], p[2], &f);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
#pragma unroll
            for (int d = 0; d < 3; ++d) u[i][d] = (p[i][d] - F.c[d]) / F.L;
        }
        const double area = tm_normal(u[0], u[1], u[2], N) * 0.5;
        a[0] += (unsigned long long)llrint(area * F.scale);
        int w = 4;
#pragma unroll
        for (int d = 0; d < 3; ++d) s[d] = (u[0][d] + u[1][d]) + u[2][d];
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            a[1 + d] += (unsigned long long)llrint((area * s[d]) * F.scale);
#pragma unroll
            for (int k = d; k < 3; ++k, ++w) {
                const double q = ((u[0][d] * u[0][k] + u[1][d] * u[1][k]) + u[2][d] * u[2][k]) + s[d] * s[k];
                a[w] += (unsigned long long)llrint((area * q) * F.scale);
            }
        }
    }
    mom_flush(a, s_a, acc);
}

/* The frame the ten words of a surface imply (B.136): m_d = S1_d / (3 W0), C_dk = S2_dk / (12 W0) - m_d m_k -- the fixed point
   cancels --, then frame_from_mean_cov.  count: the indexed triangles.  false: W0 <= 0, L not finite and > 0, ms outside [0, 62]. */
inline bool mesh_frame_from_words(const long long *words, size_t count, int ms, const double *c, double L, ppp_cloud_frame *f)
{
    if (words[0] <= 0 || !(L > 0.0) || !(L < INFINITY) || ms < 0 || ms > 62) return false;
    f->count = count; f->ms = ms; f->L = L;
    for (int d = 0; d < 3; ++d) f->c[d] = c[d];
    for (int w = 0; w < MOM_WORDS; ++w) f->words[w] = words[w];
    const double W0 = (double)words[0];
    double m[3], A[3][3];
    for (int d = 0; d < 3; ++d) m[d] = (double)words[1 + d] / (3.0 * W0);
    for (int d = 0, w = 4; d < 3; ++d)
        for (int k = d; k < 3; ++k, ++w) A[d][k] = A[k][d] = (double)words[w] / (12.0 * W0) - m[d] * m[k];
    frame_from_mean_cov(m, A, c, L, f);
    return true;
}
