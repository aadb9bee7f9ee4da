/*
 * ppp_mesh_registration.h -- point-to-plane ICP of a handle's cloud, the scan, to a resident triangle mesh
 * (ppp_get_mesh_registration_terms, ppp_register_mesh).  An evaluation: the scan's points, moved by the current
 * transform in double (icp_move), through the mesh's grid (tm_nearest: the nearest indexed triangle by (D2, f), the exact closest
 * point), the winning facet's own normal (tm_load, tm_normal), and the 29 integer sums of the normal equations (icp_add_terms on
 * doubles) -- as two launches, k_mesh_reg_search and k_mesh_reg_sum, or as the fused k_mesh_reg_terms (MESH_REG_SPLIT).  The step
 * is k_reg_step, unchanged; the host's chain has registration_chain's shape.  Nothing here estimates a normal or knows a pitch:
 * the fit is taken on the facets that ppp_get_mesh_deviation measures against.
 * Robust weights on these pairs are ppp_mesh_robust.h's; trimmed weights, tiles, a global start from the mesh,
 * pseudonormals and border rejection are not offered.
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

__global__ void __launch_bounds__(TM_T) k_mesh_reg_search(const float4 *__restrict__ q4, int nq, const TriGrid G, double md2, const double *__restrict__ T,
        const IcpCtl *__restrict__ ctl, unsigned *__restrict__ win)
{
    if (ctl->done) return;
    const int at = blockIdx.x * TM_T + threadIdx.x;
    if (at >= nq) return;
    double t[12], m[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    icp_move(t, q4[at], m);
    unsigned w = MESH_REG_NONE;
    if (isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2])) {
        TmBest B;
        tm_nearest(G, m, md2, B);
        if (B.r >= 0 && B.D2 <= md2) w = (unsigned)B.r;
    }
    win[at] = w;
}

__global__ void __launch_bounds__(ICP_T) k_mesh_reg_sum(const float4 *__restrict__ q4, int nq, const TriGrid G, const IcpFrame F, const double *__restrict__ T,
        const IcpCtl *__restrict__ ctl, const unsigned *__restrict__ win, unsigned long long *__restrict__ acc)
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
        const unsigned r = win[at];
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
