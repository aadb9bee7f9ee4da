/*
 * ppp_robust_tile.h -- robust registration of a scan held as slice-range tiles (ppp_register_robust_tiles, ppp_robust_sigma,
 * ppp_robust_weight).  Everything a robust evaluation needs merges exactly over the tiles: a pair,
 * its residual and its key are a point's own (B.101), the median is a rank statistic of the union of the keys (B.102) -- §7p's
 * three digit histograms add bin by bin --, sigma and the cut follow from the merged tau by rob_sigma and one product, which
 * the host and the device compile alike, the weight is a function of a point's own residual and that cut (B.103), and the 30
 * words are integer sums (B.104).  The kernels are the tile forms of ppp_robust.h's, over the index positions [pos0, pos1) of
 * the slabs that meet the owned interval; ppp_trimmed_tile.h's k_trimt_narrow<1> and <2> count the middle and the low digits
 * as they are: they work on any key array.  None of the kernels selects a digit and none reads IcpCtl: the loop is the
 * host's.  The keys, the partners and the residuals are stored by position - pos0.  No float atomics.
 */
#pragma once
#include "ppp_robust.h"
#include "ppp_trimmed_tile.h"

/* k_trimt_pair with k_rob_pair's residual and key, for the positions [pos0, pos1): an owned point (B.36: by its resident,
   unmoved x) is moved by T (icp_move), the float of the moved point is paired in the slabs [rb0, rb1) the reference's handle
   sorted (dev_pair: a partner whose normal holds a NaN is no pair, B.101), and a pair leaves its partner, its residual against
   the partner's normal and the key of (float)fabs(r), and counts the key's top digit in LDS; an owned point without a pair
   leaves TRIM_NONE, a position that is not owned TRIMT_HALO.  An owned query with a finite moved position whose reach leaves
   what a slice-range reference indexes is counted in head[TRIMT_REFUSED] and pairs with nothing (k_regt_terms' test): the host
   refuses the call.  head: the two words, then the top digits' histogram; flushed once per workgroup. */
__global__ void __launch_bounds__(TRIM_T) k_robt_pair(const float4 *__restrict__ q4, int pos0, int pos1, const TileRange own, const ContactIndex R,
        int nref, int rb0, int rb1, const RegtNeed need, const IcpFrame *__restrict__ Fp, const double *__restrict__ T,
        float4 *__restrict__ partner, double *__restrict__ res, u32 *__restrict__ key, u32 *__restrict__ head)
{
    __shared__ u32 s_h[TRIM_B0];
    __shared__ u32 s_x[TRIMT_HEAD];
    for (int b = threadIdx.x; b < TRIM_B0; b += TRIM_T) s_h[b] = 0;
    if (threadIdx.x < TRIMT_HEAD) s_x[threadIdx.x] = 0;
    __syncthreads();
    const float md2 = Fp->md2;
    u32 mine = 0, refused = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = pos0 + blockIdx.x * TRIM_T + threadIdx.x; at < pos1; at += gridDim.x * TRIM_T) {
        const float4 p = q4[at];
        u32 kk = TRIMT_HALO;
        if (own.owned(p.x)) {
            ++mine;
            kk = TRIM_NONE;
            double m[3];
            icp_move(t, p, m);
            const float qx = (float)m[0], qy = (float)m[1], qz = (float)m[2];
            if (isfinite(qx) && isfinite(qy) && isfinite(qz)) {
                DevPair P;
                if (need.refuses(qx)) ++refused;
                else if (dev_pair<false>(R, nref, rb0, rb1, qx, qy, qz, md2, P) == PPP_DEV_MATCHED) {
                    const double r = rob_residual(m, P.q, P.n);
                    kk = __float_as_uint((float)fabs(r));
                    partner[at - pos0] = P.q;
                    res[at - pos0] = r;
                    atomicAdd(&s_h[kk >> 21], 1u);
                }
            }
        }
        key[at - pos0] = kk;
    }
    if (mine) atomicAdd(&s_x[TRIMT_OWNED], mine);
    if (refused) atomicAdd(&s_x[TRIMT_REFUSED], refused);
    __syncthreads();
    trim_flush(s_h, TRIM_B0, head + TRIMT_HEAD);
    if (threadIdx.x < TRIMT_HEAD && s_x[threadIdx.x]) atomicAdd(head + threadIdx.x, s_x[threadIdx.x]);
}

/* k_rob_terms' loop for the positions [pos0, pos1): sigma and the cut from *tau -- the merged median, written by the host before
   the launch -- as k_rob_terms makes them in its prologue (B.107), then the 30 words over the tile's owned pairs: the moved
   point made again from T, the partner and the residual read back, rob_weight, rob_add_terms; rob_flush.  TRIM_NONE and
   TRIMT_HALO are no pair.  The host launches it only behind an evaluation that found a pair in some tile. */
__global__ void __launch_bounds__(TRIM_T) k_robt_terms(const float4 *__restrict__ q4, int pos0, int pos1, const ContactIndex R,
        const IcpFrame *__restrict__ Fp, const RobScale S, const double *__restrict__ T, const float4 *__restrict__ partner,
        const double *__restrict__ res, const u32 *__restrict__ key, const u32 *__restrict__ taup, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[TRIM_T / 64][ROB_WORDS];
    const IcpFrame F = *Fp;
    const double sigma = rob_sigma(*taup, false, S.sigma_min);
    const double cs = S.tune * sigma;
    unsigned long long a[ROB_WORDS];
#pragma unroll
    for (int w = 0; w < ROB_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = pos0 + blockIdx.x * TRIM_T + threadIdx.x; at < pos1; at += gridDim.x * TRIM_T) {
        const u32 kk = key[at - pos0];
        if (kk == TRIM_NONE || kk == TRIMT_HALO) continue;
        double m[3];
        icp_move(t, q4[at], m);
        const double r = res[at - pos0];
        rob_add_terms(a, m, r, rob_weight(r, cs, S.tune), R.normals4[idx_of(partner[at - pos0])], F);
    }
    rob_flush(a, s_a, acc);
}

/* k_rob_fill for a tile's four maps: DROPPED, the float quiet NaN, the double one and owned 0 in every entry (n >= 1) */
__global__ void __launch_bounds__(TRIM_T) k_robt_fill(int n, unsigned char *__restrict__ status, float *__restrict__ weight, double *__restrict__ residual,
        unsigned char *__restrict__ owned)
{
    for (int i = blockIdx.x * TRIM_T + threadIdx.x; i < n; i += gridDim.x * TRIM_T) {
        status[i] = PPP_ROBUST_DROPPED;
        weight[i] = __uint_as_float(TRIM_NAN);
        residual[i] = icp_nan();
        owned[i] = 0;
    }
}

/* k_rob_scatter for a tile, once behind the loop (B.109): the keys and the residuals are the last evaluation's, cs its merged
   cut -- tune times the host's rob_sigma of the merged tau --, none: it found no pair in any tile.  An owned indexed point
   writes its own entries of the maps by cloud index and owned[id] = 1; the maps hold DROPPED / NaN / NaN / 0 before the launch
   (k_robt_fill), which every other entry keeps -- a position that is not owned among them. */
__global__ void __launch_bounds__(TRIM_T) k_robt_scatter(const float4 *__restrict__ q4, int pos0, int pos1, const u32 *__restrict__ key,
        const double *__restrict__ res, double cs, double tune, int none, int cap, unsigned char *__restrict__ status, float *__restrict__ weight,
        double *__restrict__ residual, unsigned char *__restrict__ owned)
{
    for (int at = pos0 + blockIdx.x * TRIM_T + threadIdx.x; at < pos1; at += gridDim.x * TRIM_T) {
        const u32 kk = key[at - pos0];
        if (kk == TRIMT_HALO) continue;
        const int id = idx_of(q4[at]);
        if (id < 0 || id >= cap) continue;
        owned[id] = 1;
        if (kk == TRIM_NONE || none) { status[id] = PPP_ROBUST_UNPAIRED; continue; }
        const double r = res[at - pos0];
        const double w = rob_weight(r, cs, tune);
        status[id] = w > 0.0 ? PPP_ROBUST_USED : PPP_ROBUST_REJECTED;
        weight[id] = (float)w;
        residual[id] = r;
    }
}
