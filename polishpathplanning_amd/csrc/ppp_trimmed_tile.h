/*
 * ppp_trimmed_tile.h -- trimmed registration of a scan held as slice-range tiles (ppp_register_trimmed_tiles, ppp_trim_select,
 * ppp_trim_rank).  Every quantity of a trimmed evaluation is an integer histogram or an integer sum:
 * pairs and keys are a point's own (B.77), the cut is a rank statistic of the union of the keys (B.78), the 29 words add (B.91).
 * The kernels are the tile forms of ppp_trimmed.h's four, over the index positions [pos0, pos1) of the slabs that meet the owned
 * interval; a tile's histograms count its owned points' keys only, the host adds the tiles' histograms bin by bin, selects the
 * digit on the merged one (ppp_trim_select: trim_select's rule) and hands every tile the merged prefix, then tau, in device
 * memory.  None of them selects a digit and none reads IcpCtl: the loop is the host's.  The keys and the partners are stored by
 * position - pos0.  No float atomics.
 */
#pragma once
#include "ppp_trimmed.h"
#include "ppp_registration_tile.h"

/* the key of a position the tile does not own: its top digit is 2 047, which no pair's key has (a finite float's is at most
   1 019), so no pass counts it; it lies above every tau, so it is never kept; and k_trimt_scatter passes it by */
#define TRIMT_HALO 0xfffffffeu
/* the words in front of a tile's three histograms: the owned points met, the owned queries that set the refusal (B.89) */
#define TRIMT_OWNED 0
#define TRIMT_REFUSED 1
#define TRIMT_HEAD 2

/* k_trim_pair for the positions [pos0, pos1): an owned point (B.36: by its resident, unmoved x) is moved by T (icp_move), the
   float of the moved point is paired in the slabs [rb0, rb1) the reference's handle sorted (dev_pair), and a pair leaves its
   partner and its key and counts the key's top digit in LDS; an owned point without a pair leaves TRIM_NONE, a position that is
   not owned TRIMT_HALO.  An owned query with a finite moved position whose reach leaves what a slice-range reference indexes
   is counted in head[TRIMT_REFUSED] and pairs with nothing (k_regt_terms' test): the host refuses the call.  head: the two
   words, then the top digits' histogram; flushed once per workgroup. */
__global__ void __launch_bounds__(TRIM_T) k_trimt_pair(const float4 *__restrict__ q4, int pos0, int pos1, const TileRange own, const ContactIndex R,
        int nref, int rb0, int rb1, const RegtNeed need, const IcpFrame *__restrict__ Fp, const double *__restrict__ T,
        float4 *__restrict__ partner, u32 *__restrict__ key, u32 *__restrict__ head)
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
                    kk = __float_as_uint(P.d2);
                    partner[at - pos0] = P.q;
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

/* k_trim_narrow's counting loop over the tile's n stored keys: PASS 1 counts bits 20..10 of the keys that carry the top digit
   of *prefix, PASS 2 bits 9..0 of the keys that carry its top and middle digits.  *prefix is the merged histogram's, written by
   the host before the launch. */
template <int PASS>
__global__ void __launch_bounds__(TRIM_T) k_trimt_narrow(const u32 *__restrict__ key, int n, const u32 *__restrict__ prefixp, u32 *__restrict__ next)
{
    constexpr int BINS = PASS == 1 ? TRIM_B1 : TRIM_B2;
    __shared__ u32 s_h[BINS];
    for (int b = threadIdx.x; b < BINS; b += TRIM_T) s_h[b] = 0;
    __syncthreads();
    const u32 prefix = *prefixp;
    const u32 mask = PASS == 1 ? 0xffe00000u : 0xfffffc00u;
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < n; at += gridDim.x * TRIM_T) {
        const u32 kk = key[at];
        if ((kk & mask) == prefix) atomicAdd(&s_h[PASS == 1 ? (kk >> 10) & (TRIM_B1 - 1) : kk & (TRIM_B2 - 1)], 1u);
    }
    __syncthreads();
    trim_flush(s_h, BINS, next);
}

/* k_trim_terms' loop for the positions [pos0, pos1): the 29 words (icp_add_terms) over the keys <= *tau -- the merged cut,
   written by the host before the launch --, the moved point made again from T, the partner and the key read back; icp_flush.
   TRIM_NONE and TRIMT_HALO lie above every cut. */
__global__ void __launch_bounds__(TRIM_T) k_trimt_terms(const float4 *__restrict__ q4, int pos0, int pos1, const ContactIndex R,
        const IcpFrame *__restrict__ Fp, const double *__restrict__ T, const float4 *__restrict__ partner, const u32 *__restrict__ key,
        const u32 *__restrict__ taup, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[TRIM_T / 64][ICP_WORDS];
    const IcpFrame F = *Fp;
    const u32 tau = *taup;
    unsigned long long a[ICP_WORDS];
#pragma unroll
    for (int w = 0; w < ICP_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = pos0 + blockIdx.x * TRIM_T + threadIdx.x; at < pos1; at += gridDim.x * TRIM_T) {
        if (key[at - pos0] > tau) continue;
        double m[3];
        icp_move(t, q4[at], m);
        const float4 q = partner[at - pos0];
        icp_add_terms(a, m, q, R.normals4[idx_of(q)], F);
    }
    icp_flush<TRIM_T>(a, s_a, acc);
}

/* k_trim_scatter for a tile, once behind the loop: the keys are the last evaluation's, tau its merged cut, none: it found no
   pair in any tile.  An owned indexed point writes its own entries of the maps by cloud index and owned[id] = 1; the maps hold
   DROPPED / NaN / 0 before the launch, which every other entry keeps -- a position that is not owned among them. */
__global__ void __launch_bounds__(TRIM_T) k_trimt_scatter(const float4 *__restrict__ q4, int pos0, int pos1, const u32 *__restrict__ key, u32 tau, int none,
        int cap, unsigned char *__restrict__ status, float *__restrict__ d2, unsigned char *__restrict__ owned)
{
    for (int at = pos0 + blockIdx.x * TRIM_T + threadIdx.x; at < pos1; at += gridDim.x * TRIM_T) {
        const u32 kk = key[at - pos0];
        if (kk == TRIMT_HALO) continue;
        const int id = idx_of(q4[at]);
        if (id < 0 || id >= cap) continue;
        owned[id] = 1;
        if (kk == TRIM_NONE || none) { status[id] = PPP_TRIM_UNPAIRED; continue; }
        status[id] = kk <= tau ? PPP_TRIM_KEPT : PPP_TRIM_TRIMMED;
        d2[id] = __uint_as_float(kk);
    }
}
