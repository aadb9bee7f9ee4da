/*
 * ppp_mesh_tile.h -- the exact deviation and the plain registration against a resident triangle mesh for the points a handle owns
 * (ppp_get_mesh_deviation_tile, ppp_get_mesh_signed_deviation_tile, ppp_get_mesh_registration_terms_tile,
 * ppp_register_mesh_tiles): the tile forms of ppp_trimesh.h's, ppp_trimesh_topology.h's and
 * ppp_mesh_registration.h's kernels.  The mesh is whole on every device, so nothing on the reference's side needs a halo or a
 * range test; a tile evaluates the scan's indexed points in the owned interval widened by smooth_radius (ppp_deviation_tile.h's
 * W(r)) -- the positions [pos0, pos1) of the slabs that meet it -- and reports the owned ones.  The per-query bodies are the
 * whole-cloud kernels' own (mesh_nearest_body, mesh_sign_body, mesh_reg_search_body, mesh_reg_sum_body): an owned point's entries
 * and words are the same bits.  The smoothing and the target are ppp_deviation_tile.h's k_devt_smooth and k_devt_target as they
 * are.  Partial statistics by integer atomics, one per workgroup and non-zero word.  No float atomics.
 */
#pragma once
#include "ppp_deviation_tile.h"
#include "ppp_trimesh.h"
#include "ppp_trimesh_topology.h"
#include "ppp_mesh_registration.h"
#include "ppp_registration_tile.h"

/* What every map holds for a point the tile does not report, a thread per cloud index (grid-stride): k_devt_fill's values and
   those of k_tm_fill and k_tm_sign_fill -- DROPPED, -1, 255, the NaN, +0, flags 0, owned 0.  smoothed: NULL without smoothing;
   feature, flags: NULL in the unsigned call. */
__global__ void __launch_bounds__(TM_T) k_mesht_fill(int n, double *__restrict__ deviation, double *__restrict__ smoothed, double *__restrict__ target,
        double *__restrict__ distance, int *__restrict__ tri_index, unsigned char *__restrict__ region, unsigned char *__restrict__ feature,
        unsigned char *__restrict__ flags, unsigned char *__restrict__ status, unsigned char *__restrict__ owned)
{
    for (int i = blockIdx.x * TM_T + threadIdx.x; i < n; i += gridDim.x * TM_T) {
        deviation[i] = dev_nan(); target[i] = 0.0; distance[i] = dev_nan(); tri_index[i] = -1; region[i] = 255; status[i] = PPP_DEV_DROPPED; owned[i] = 0;
        if (smoothed) smoothed[i] = dev_nan();
        if (feature) { feature[i] = 255; flags[i] = 0; }
    }
}

/* k_mesh_nearest for the positions [pos0, pos1) of the scan's index: a thread per position, the evaluated ones (T) through
   mesh_nearest_body.  An owned point gets every entry and owned[id] = 1; a halo point gets what the smoothing and the sign
   kernel read -- status, tri_index, deviation, its fixed-point term, d2 -- and keeps the fill's distance and region: k_devt_target
   takes the first three back, nothing else of it is reported. */
__global__ void __launch_bounds__(TM_T) k_mesht_nearest(const float4 *__restrict__ q4, int pos0, int pos1, TileRange T, const TriGrid G, double md2, TmOut O,
        unsigned char *__restrict__ owned)
{
    const int t = pos0 + blockIdx.x * TM_T + threadIdx.x;
    if (t >= pos1) return;
    const float4 q = q4[t];
    if (!T.evaluated(q.x)) return;
    const int id = idx_of(q);
    if (T.owned(q.x)) owned[id] = 1;
    else { O.distance = nullptr; O.region = nullptr; }
    mesh_nearest_body(q.x, q.y, q.z, id, G, md2, O);
}

/* k_mesh_sign for the same positions, behind k_mesht_nearest: every evaluated point's deviation and fixed-point term are
   rewritten with the signed distance (the halo's enter the owned points' smoothing sums); feature and flags are the owned
   points' alone. */
__global__ void __launch_bounds__(TM_T) k_mesht_sign(const float4 *__restrict__ q4, int pos0, int pos1, TileRange T, const TriGrid G, const TriTopo Tp, TmSignOut O)
{
    const int t = pos0 + blockIdx.x * TM_T + threadIdx.x;
    if (t >= pos1) return;
    const float4 q = q4[t];
    if (!T.evaluated(q.x)) return;
    if (!T.owned(q.x)) { O.feature = nullptr; O.flags = nullptr; }
    mesh_sign_body(q.x, q.y, q.z, idx_of(q), G, Tp, O);
}

/* The accumulators of a tile beside k_devt_target's: k_tm_region_stats' four words -- the owned matched points by region and the
   largest distance's bits -- and k_tm_sign_stats' five behind them (the signed call: flags != NULL). */
#define MESHT_ACC_FAR 3
#define MESHT_ACC_SIGN 4
#define MESHT_ACC_WORDS 9

/* k_tm_region_stats and k_tm_sign_stats over the OWNED points of [pos0, pos1), grid-stride, behind the search (and the sign
   kernel): wave, workgroup (LDS), one integer atomic per workgroup and non-zero word. */
__global__ void __launch_bounds__(TM_T) k_mesht_stats(const float4 *__restrict__ q4, int pos0, int pos1, TileRange T, const unsigned char *__restrict__ status,
        const unsigned char *__restrict__ region, const double *__restrict__ distance, const unsigned char *__restrict__ flags,
        const double *__restrict__ signed_distance, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[MESHT_ACC_WORDS];
    if (threadIdx.x < MESHT_ACC_WORDS) s_a[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long cnt[MESHT_ACC_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int t = pos0 + blockIdx.x * TM_T + threadIdx.x; t < pos1; t += gridDim.x * TM_T) {
        const float4 q = q4[t];
        if (!T.owned(q.x)) continue;
        const int i = idx_of(q);
        if (status[i] != PPP_DEV_MATCHED) continue;
        const int g = region[i];
        cnt[0] += g == 0; cnt[1] += g == 1; cnt[2] += g == 2;
        cnt[MESHT_ACC_FAR] = max(cnt[MESHT_ACC_FAR], (unsigned long long)__double_as_longlong(distance[i]));
        if (flags) {
            const int fl = flags[i];
            const double v = signed_distance[i];
            cnt[MESHT_ACC_SIGN] += (fl & PPP_MESH_SIGN_BORDER) != 0; cnt[MESHT_ACC_SIGN + 1] += (fl & PPP_MESH_SIGN_IRREGULAR) != 0;
            cnt[MESHT_ACC_SIGN + 2] += (fl & PPP_MESH_SIGN_FALLBACK) != 0;
            cnt[MESHT_ACC_SIGN + 3] += v < 0.0; cnt[MESHT_ACC_SIGN + 4] += v > 0.0;
        }
    }
#pragma unroll
    for (int k = 0; k < MESHT_ACC_WORDS; ++k) {
        cnt[k] = k == MESHT_ACC_FAR ? wave_max_bits(cnt[k]) : wave_sum(cnt[k]);
        if ((threadIdx.x & 63) == 0 && cnt[k]) {
            if (k == MESHT_ACC_FAR) atomicMax(&s_a[k], cnt[k]); else atomicAdd(&s_a[k], cnt[k]);
        }
    }
    __syncthreads();
    if (threadIdx.x < MESHT_ACC_WORDS && s_a[threadIdx.x]) {
        if (threadIdx.x == MESHT_ACC_FAR) atomicMax(acc + threadIdx.x, s_a[threadIdx.x]); else atomicAdd(acc + threadIdx.x, s_a[threadIdx.x]);
    }
}

/* The split evaluation of ppp_mesh_registration.h over the positions [pos0, pos1) (B.148): k_mesht_reg_search is a thread per
   position -- win[at - pos0] = the winning record of an owned point moved by T, MESH_REG_NONE for a position that is not owned or
   has no pair --, k_mesht_reg_sum the grid-stride sum into acc[0 .. 28] with the owned positions counted into acc[REGT_OWNED], as
   k_regt_terms counts them.  T is read from device memory: the host writes it before every evaluation of the loop. */
__global__ void __launch_bounds__(TM_T) k_mesht_reg_search(const float4 *__restrict__ q4, int pos0, int pos1, const TileRange own, const TriGrid G, double md2,
        const double *__restrict__ T, unsigned *__restrict__ win)
{
    mesh_reg_search_body<true>(q4, pos0, pos1, own, G, md2, T, win, pos0 + blockIdx.x * TM_T + threadIdx.x);
}

__global__ void __launch_bounds__(ICP_T) k_mesht_reg_sum(const float4 *__restrict__ q4, int pos0, int pos1, const TileRange own, const TriGrid G,
        const IcpFrame *__restrict__ Fp, const double *__restrict__ T, const unsigned *__restrict__ win, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_x[ICP_T / 64];
    const IcpFrame F = *Fp;
    unsigned long long mine = 0;
    mesh_reg_sum_body<true>(q4, pos0, pos1, own, G, F, T, win, acc, blockIdx.x, gridDim.x, &mine);
    mine = wave_sum(mine);
    if ((threadIdx.x & 63) == 0) s_x[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s = 0;
        for (int v = 0; v < ICP_T / 64; ++v) s += s_x[v];
        if (s) atomicAdd(acc + REGT_OWNED, s);
    }
}
