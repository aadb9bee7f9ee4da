/*
 * ppp_mesh_trimmed.h -- trimmed registration of a handle's cloud, the scan, to a resident triangle mesh, with border-pair
 * rejection (ppp_get_mesh_trimmed_registration_terms, ppp_register_mesh_trimmed): ppp_register_mesh's
 * candidates -- the moved point in double, the nearest indexed triangle by (D2, f), its exact closest point -- under
 * ppp_register_trimmed's cut: the key of (float)D2, the rank ppp_trim_rank(keep, paired) through ppp_trimmed.h's three digit
 * histograms, and ppp_register_mesh's 29 words over the pairs with key <= tau.  Under PPP_MESH_BORDER_REJECT a candidate whose
 * closest point lies on a border edge or a border vertex of the welded topology (ppp_trimesh_topology.h) is no pair: the
 * condition under which k_mesh_sign sets PPP_MESH_SIGN_BORDER.  An evaluation pays the grid walk once: k_mesh_trim_pair (the
 * walk, a thread per query: the winning record and the key), k_mesh_trim_digit0 (the top digit's counts over the stored keys,
 * and the count of the border's rejects), k_trim_narrow<1> and <2> as they are, k_mesh_trim_terms (tau, the sums over the stored
 * winners) and k_reg_step, unchanged.  k_mesh_trim_scatter, once behind the chain, makes the status and d2 maps.
 * The walk and the 29 accumulators never share a kernel.  The facet's orientation is not applied:
 * ppp_mesh_registration.h's reason; the class of an edge with one half-edge does not depend on a direction either.
 */
#pragma once
#include "ppp_trimmed.h"
#include "ppp_mesh_registration.h"
#include "ppp_trimesh_topology.h"

/* the key of a candidate the border rule rejected: beside TRIM_NONE in the negative NaNs, above every float that is no NaN, so
   no prefix k_trim_narrow finds -- a bin with a count in it -- can match either (B.142) */
#define MESH_TRIM_BORDER 0xfffffffeu
static_assert(MESH_TRIM_BORDER < TRIM_NONE && MESH_TRIM_BORDER > 0xff800000u, "the border's key is a NaN's pattern below TRIM_NONE");

/* the workgroups of k_mesh_trim_terms are capped at MESH_TRIM_GRID_CUS per compute unit, as k_mesh_reg_sum's are under
   MESH_REG_GRID_CUS (0: no cap); integer sums make the words independent of it */
#ifndef MESH_TRIM_GRID_CUS
#define MESH_TRIM_GRID_CUS MESH_REG_GRID_CUS
#endif

/* B.140, B.141: k_mesh_reg_search's walk, a thread per indexed point of the scan in slab order (q4 = its sorted4, nq = its
   n_sorted).  A candidate (B.r >= 0 and D2 <= md2, inclusive) leaves the winning record's number and the key of (float)D2, the
   walk's double narrowed once; any other query the key TRIM_NONE.  REJECT: the winner's record is walked once more with
   tm_closest_feature -- the same inputs, the same arithmetic: its feature belongs to the walk's x -- and a candidate on a vertex
   with PPP_VERTEX_BORDER or on an edge of class PPP_EDGE_BORDER leaves the key MESH_TRIM_BORDER instead.  The rule is a
   template parameter: the PAIR form reads no topology and carries none of its registers.  No sums here. */
template <bool REJECT>
__global__ void __launch_bounds__(TM_T) k_mesh_trim_pair(const float4 *__restrict__ q4, int nq, const TriGrid G, const TriTopo Tp, double md2,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, unsigned *__restrict__ win, u32 *__restrict__ key)
{
    if (ctl->done) return;
    const int at = blockIdx.x * TM_T + threadIdx.x;
    if (at >= nq) return;
    double t[12], m[3];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    icp_move(t, q4[at], m);
    u32 kk = TRIM_NONE;
    if (isfinite(m[0]) && isfinite(m[1]) && isfinite(m[2])) {
        TmBest B;
        tm_nearest(G, m, md2, B);
        if (B.r >= 0 && B.D2 <= md2) {
            kk = __float_as_uint((float)B.D2);
            win[at] = (unsigned)B.r;
            if (REJECT) {
                double p0[3], p1[3], p2[3], x[3], D2;
                int f, feat;
                tm_load(G.rec, B.r, p0, p1, p2, &f);
                (void)tm_closest_feature(m, p0, p1, p2, x, &D2, &feat);
                if (feat < 6) {
                    const int s = Tp.table[6 * (size_t)B.r + feat];
                    const bool border = feat < 3 ? (Tp.vbits[s] & (unsigned)PPP_VERTEX_BORDER) != 0 : Tp.eclass[s] == PPP_EDGE_BORDER;
                    if (border) kk = MESH_TRIM_BORDER;
                }
            }
        }
    }
    key[at] = kk;
}

/* the top digits of the stored keys, grid-stride, an LDS histogram per workgroup, one flush (k_mesh_rob_digit0's pass): a key
   below MESH_TRIM_BORDER is a pair's; the border's rejects are counted beside them, a wave's count at a time, into the
   evaluation's own word (*on_border: TrimCut's spare word, which no other kernel writes) */
__global__ void __launch_bounds__(TRIM_T) k_mesh_trim_digit0(const u32 *__restrict__ key, int nq, const IcpCtl *__restrict__ ctl, u32 *__restrict__ hist0,
        u32 *on_border)
{
    if (ctl->done) return;
    __shared__ u32 s_h[TRIM_B0];
    for (int b = threadIdx.x; b < TRIM_B0; b += TRIM_T) s_h[b] = 0;
    __syncthreads();
    u32 rejected = 0;
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        const u32 kk = key[at];
        if (kk < MESH_TRIM_BORDER) atomicAdd(&s_h[kk >> 21], 1u);
        else if (kk == MESH_TRIM_BORDER) ++rejected;
    }
    rejected = wave_sum(rejected);
    if ((threadIdx.x & 63) == 0 && rejected) atomicAdd(on_border, rejected);
    __syncthreads();
    trim_flush(s_h, TRIM_B0, hist0);
}

/* B.78's last digit on these keys and B.129's words: tau from hist (k_trim_narrow<2>'s counts) at the rank it left, then
   k_mesh_reg_sum's terms over the queries with key <= tau, grid-stride -- the point moved again from T (icp_move), tm_closest on
   the stored record: the same operations on the same operands, so x is the walk's bits --, icp_add_terms on doubles and
   icp_flush.  Both sentinels lie above every tau.  acc[ICP_PAIRS] is `kept`. */
__global__ void __launch_bounds__(TRIM_T) k_mesh_trim_terms(const float4 *__restrict__ q4, int nq, const TriGrid G, const IcpFrame F,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, const unsigned *__restrict__ win, const u32 *__restrict__ key, const u32 *hist,
        TrimCut *cut, unsigned long long *__restrict__ acc)
{
    if (ctl->done) return;
    static_assert(TRIM_T == ICP_T, "icp_flush's LDS rows are ICP_T / 64");
    __shared__ unsigned long long s_a[TRIM_T / 64][ICP_WORDS];
    __shared__ int s_scr[16];
    __shared__ u32 s_out[4];
    if (cut->paired == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) cut->tau = TRIM_NAN;
        return;
    }
    trim_select<TRIM_B2 / TRIM_T>(hist, false, 0.0, cut->rank2, s_scr, s_out);
    const u32 tau = cut->prefix2 | s_out[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) cut->tau = tau;
    unsigned long long a[ICP_WORDS];
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        if (key[at] > tau) continue;
        const unsigned r = win[at];
        if (r >= (unsigned)G.indexed) continue; /* (never: a key that is no sentinel has its record beside it) */
        double m[3], p0[3], p1[3], p2[3], N[3], x[3], D2;
        int f;
        icp_move(t, q4[at], m);
        tm_load(G.rec, (int)r, p0, p1, p2, &f);
        (void)tm_closest(m, p0, p1, p2, x, &D2);
        const double A2 = tm_normal(p0, p1, p2, N);
        const double n[3] = {N[0] / A2, N[1] / A2, N[2] / A2};
        icp_add_terms(a, m, x, n, F);
    }
    icp_flush<TRIM_T>(a, s_a, acc);
}

/* k_trim_scatter with the border's status (B.143): once behind the chain, the keys of the last evaluation that ran --
   evaluation ctl->steps -- and its cut.  A thread per indexed point in slab order writes its own entries of the maps by cloud
   index; they hold DROPPED / NaN before the launch, which the points outside the index keep, and a reject keeps the NaN. */
__global__ void __launch_bounds__(TRIM_T) k_mesh_trim_scatter(const float4 *__restrict__ q4, int nq, const u32 *__restrict__ key,
        const IcpCtl *__restrict__ ctl, const TrimCut *__restrict__ cuts, int evals, int cap, unsigned char *__restrict__ status, float *__restrict__ d2)
{
    const int last = ctl->steps;
    if (last < 0 || last >= evals) return; /* the host reports the control words as corrupt */
    const u32 tau = cuts[last].tau;
    const bool none = cuts[last].paired == 0;
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        const int id = idx_of(q4[at]);
        if (id < 0 || id >= cap) continue;
        const u32 kk = key[at];
        if (kk == MESH_TRIM_BORDER) { status[id] = PPP_MESH_TRIM_BORDER; continue; }
        if (kk == TRIM_NONE || none) { status[id] = PPP_TRIM_UNPAIRED; continue; }
        status[id] = kk <= tau ? PPP_TRIM_KEPT : PPP_TRIM_TRIMMED;
        d2[id] = __uint_as_float(kk);
    }
}
