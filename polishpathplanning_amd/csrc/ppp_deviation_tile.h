/*
 * ppp_deviation_tile.h -- the deviation map of the points a handle owns (ppp_get_deviation_tile): the
 * tile forms of ppp_deviation.h's kernels.  A tile evaluates the indexed points of the scan with x in the owned interval widened by smooth_radius (B.82: [own_lo - r,
 * own_hi + r] with room for the roundings) -- the positions [pos0, pos1) of the slabs that meet that interval -- and reports the owned ones; the
 * searches walk the slabs [b0, b1) that the searched handle sorted and no others: a slice-range handle keeps the whole cloud's
 * slab grid and leaves the slabs outside its interval empty, thousands of them on a large cloud.  Same minima over (distance,
 * index), same integer sums, same written operations as the whole-cloud kernels: an owned point's entries are the same bits.
 * Partial statistics by integer atomics, one per workgroup and non-zero word.  No float atomics.
 */
#pragma once
#include "ppp_deviation.h"

/* What every map holds for a point the tile does not report, a thread per cloud index (grid-stride): DROPPED, -1, the NaN,
   +0, owned 0.  The launches behind it write the evaluated points' entries.  smoothed: NULL without smoothing. */
__global__ void __launch_bounds__(DEV_T) k_devt_fill(int n, double *__restrict__ deviation, double *__restrict__ smoothed,
        double *__restrict__ target, int *__restrict__ ref_index, unsigned char *__restrict__ status, unsigned char *__restrict__ owned)
{
    for (int i = blockIdx.x * DEV_T + threadIdx.x; i < n; i += gridDim.x * DEV_T) {
        deviation[i] = dev_nan(); target[i] = 0.0; ref_index[i] = -1; status[i] = PPP_DEV_DROPPED; owned[i] = 0;
        if (smoothed) smoothed[i] = dev_nan();
    }
}

/* k_dev_nearest for the positions [pos0, pos1) of the scan's index: a thread per query in slab order, the evaluated ones (T)
   paired (dev_pair, dev_entry) in the slabs [rb0, rb1) of the reference's index R -- the slabs its handle sorted; a reference
   range handle's points carry their whole-cloud indices, so the tie rule and ref_index are the whole reference's.  owned[id] = 1
   for the tile's own. */
__global__ void __launch_bounds__(DEV_T) k_devt_nearest(const float4 *__restrict__ q4, int pos0, int pos1, TileRange T, const ContactIndex R,
        int nref, int rb0, int rb1, float md2, double *__restrict__ dev, long long *__restrict__ fix, float *__restrict__ d2,
        int *__restrict__ ref_index, unsigned char *__restrict__ status, unsigned char *__restrict__ owned)
{
    for (int t = pos0 + blockIdx.x * DEV_T + threadIdx.x; t < pos1; t += gridDim.x * DEV_T) {
        const float4 p = q4[t];
        if (!T.evaluated(p.x)) continue;
        const int id = idx_of(p);
        if (T.owned(p.x)) owned[id] = 1;
        DevPair P;
        const int st = dev_pair<false>(R, nref, rb0, rb1, p.x, p.y, p.z, md2, P);
        dev_entry(p, id, st, P, dev, fix, d2, ref_index, status);
    }
}

/* k_dev_smooth for the OWNED matched points of [pos0, pos1): dev_smooth_at over the slabs [hb0, hb1) the scan's handle sorted;
   the matched halo points it finds -- evaluated by k_devt_nearest -- take part in the integer sum. */
__global__ void __launch_bounds__(DEV_T) k_devt_smooth(const ContactIndex H, int pos0, int pos1, TileRange T, int hb0, int hb1, float r2,
        const unsigned char *__restrict__ status, const long long *__restrict__ fix, double *__restrict__ smoothed)
{
    const SlabView V = H.view();
    for (int at = pos0 + blockIdx.x * DEV_T + threadIdx.x; at < pos1; at += gridDim.x * DEV_T) {
        const float4 p = V.sorted4[at];
        if (!T.owned(p.x)) continue;
        const int id = idx_of(p);
        if (status[id] != PPP_DEV_MATCHED) continue;
        smoothed[id] = dev_smooth_at(V, hb0, hb1, at, p, r2, status, fix);
    }
}

/* The accumulators of a tile: k_dev_target's words [0 .. 9] over the OWNED points -- except [3]: an owned point is indexed, so
   never DROPPED, and the word counts the evaluated halo points instead. */
#define DEVT_ACC_HALO 3
#define DEVT_ACC_WORDS DEV_ACC_BINS

/* k_dev_target for the positions [pos0, pos1), grid-stride: an owned matched point gets its target and enters the partial
   statistics; an evaluated halo point goes back to what k_devt_fill wrote -- its deviation has served the smoothing and is
   reported nowhere.  (Every other entry of a point that is not matched still holds the fill's value.)  Without smoothing v IS
   deviation: the two are not restrict.  The reduction is k_dev_target's: DevTargetAcc. */
__global__ void __launch_bounds__(DEV_T) k_devt_target(const float4 *__restrict__ sorted4, int pos0, int pos1, TileRange T,
        unsigned char *__restrict__ status, double *deviation, const double *v, const float *__restrict__ d2, int *__restrict__ ref_index,
        double allowance, double gain, double *__restrict__ target, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[DEV_ACC_BINS];
    if (threadIdx.x < DEV_ACC_BINS) s_a[threadIdx.x] = 0;
    __syncthreads();
    DevTargetAcc a;
    for (int pos = pos0 + blockIdx.x * DEV_T + threadIdx.x; pos < pos1; pos += gridDim.x * DEV_T) {
        const float4 p = sorted4[pos];
        if (!T.evaluated(p.x)) continue;
        const int i = idx_of(p);
        if (!T.owned(p.x)) {
            ++a.cnt[DEVT_ACC_HALO];
            status[i] = PPP_DEV_DROPPED; ref_index[i] = -1; deviation[i] = dev_nan();
            continue;
        }
        const int st = status[i];
        a.cnt[0] += st == PPP_DEV_MATCHED; a.cnt[1] += st == PPP_DEV_TOO_FAR; a.cnt[2] += st == PPP_DEV_NO_NORMAL;
        if (st != PPP_DEV_MATCHED) continue;
        const double x = v[i], over = x - allowance;
        target[i] = over > 0.0 ? gain * over : 0.0;
        a.add(x, allowance, d2[i]);
    }
    a.flush(s_a, acc);
}
