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

/* dev_nearest_within over the slabs [b0, b1) of V alone (0, B: the whole index).  The slab of the query may lie outside them:
   it is then empty, and either walk starts at the nearer end of the interval. */
__device__ inline int devt_nearest_within(const SlabView &V, int b0, int b1, float qx, float qy, float qz, float bound2, float4 *found,
                                          float *d2)
{
    float best = bound2;
    int bidx = 0x7fffffff;
    float4 bp = make_float4(NAN, NAN, NAN, 0.f);
    auto visit = [&](const float4 &c) {
        const float dy = qy - c.y;
        if (dy * dy > best) return false;
        const float d = dist2_flann(qx, qy, qz, c.x, c.y, c.z);
        const int id = idx_of(c);
        if (d < best || (d == best && id < bidx)) { best = d; bidx = id; bp = c; }
        return true;
    };
    auto scan_slab = [&](int bb, int s0, int s1) {
        int lo, hi;
        V.narrow(bb, s0, s1, qy, lo, hi);
        const int p = lower_bound_y(V, lo, hi, qy);
        for (int i = p; i < s1; ++i) if (!visit(V.sorted4[i])) break;
        for (int i = p - 1; i >= s0; --i) if (!visit(V.sorted4[i])) break;
    };
    const int b = slab_of(V.m, qx);
    if (b >= b0 && b < b1) {
        const int s0 = V.slab_start[b], s1 = V.slab_start[b + 1];
        if (s0 < s1) scan_slab(b, s0, s1);
    }
    for (int bb = max(b + 1, b0); bb < b1; ++bb) {
        const int s0 = V.slab_start[bb], s1 = V.slab_start[bb + 1];
        if (s0 >= s1) continue;
        const float dx = V.slab_xmin[bb] - qx;
        if (dx > 0.f && dx * dx > best) break;
        scan_slab(bb, s0, s1);
    }
    for (int bb = min(b - 1, b1 - 1); bb >= b0; --bb) {
        const int s0 = V.slab_start[bb], s1 = V.slab_start[bb + 1];
        if (s0 >= s1) continue;
        const float dx = qx - V.slab_xmax[bb];
        if (dx > 0.f && dx * dx > best) break;
        scan_slab(bb, s0, s1);
    }
    *found = bp; *d2 = best;
    return bidx == 0x7fffffff ? -1 : bidx;
}

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
   searched in the slabs [rb0, rb1) of the reference's index R -- the slabs its handle sorted; a reference range handle's points
   carry their whole-cloud indices, so the tie rule and ref_index are the whole reference's.  owned[id] = 1 for the tile's own. */
__global__ void __launch_bounds__(DEV_T) k_devt_nearest(const float4 *__restrict__ q4, int pos0, int pos1, TileRange T, const ContactIndex R,
        int nref, int rb0, int rb1, float md2, double *__restrict__ dev, long long *__restrict__ fix, float *__restrict__ d2,
        int *__restrict__ ref_index, unsigned char *__restrict__ status, unsigned char *__restrict__ owned)
{
    for (int t = pos0 + blockIdx.x * DEV_T + threadIdx.x; t < pos1; t += gridDim.x * DEV_T) {
        const float4 p = q4[t];
        if (!T.evaluated(p.x)) continue;
        const int id = idx_of(p);
        if (T.owned(p.x)) owned[id] = 1;
        float4 q = make_float4(NAN, NAN, NAN, 0.f);
        float dd = NAN;
        const int j = nref > 0 ? devt_nearest_within(R.view(), rb0, rb1, p.x, p.y, p.z, md2, &q, &dd) : -1;
        if (j < 0) { status[id] = PPP_DEV_TOO_FAR; continue; }
        ref_index[id] = j;
        const float4 n = R.normals4[j];
        if (!(n.x == n.x && n.y == n.y && n.z == n.z && n.w == n.w)) { status[id] = PPP_DEV_NO_NORMAL; continue; }
        const double ex = (double)p.x - (double)q.x, ey = (double)p.y - (double)q.y, ez = (double)p.z - (double)q.z;
        const double v = ((ex * (double)n.x) + ey * (double)n.y) + ez * (double)n.z;
        status[id] = PPP_DEV_MATCHED;
        dev[id] = v; d2[id] = dd; fix[id] = llrint(v * DEV_FIXED);
    }
}

/* k_dev_smooth for the OWNED matched points of [pos0, pos1): the ball of r2 in the scan's own index, walked over the slabs
   [hb0, hb1) its handle sorted; the matched halo points it finds -- evaluated by k_devt_nearest -- take part in the integer sum. */
__global__ void __launch_bounds__(DEV_T) k_devt_smooth(const ContactIndex H, int pos0, int pos1, TileRange T, int hb0, int hb1, float r2,
        const unsigned char *__restrict__ status, const long long *__restrict__ fix, double *__restrict__ smoothed)
{
    const SlabView V = H.view();
    for (int at = pos0 + blockIdx.x * DEV_T + threadIdx.x; at < pos1; at += gridDim.x * DEV_T) {
        const float4 p = V.sorted4[at];
        if (!T.owned(p.x)) continue;
        const int id = idx_of(p);
        if (status[id] != PPP_DEV_MATCHED) continue;
        long long sum = 0;
        int cnt = 0;
        auto scan_from = [&](int s0, int s1, int q0) {
            auto visit = [&](const float4 &c) {
                const float dy = p.y - c.y;
                if (dy * dy > r2) return false;
                const int k = idx_of(c);
                if (dist2_flann(p.x, p.y, p.z, c.x, c.y, c.z) <= r2 && status[k] == PPP_DEV_MATCHED) { sum += fix[k]; ++cnt; }
                return true;
            };
            for (int i = q0; i < s1; ++i) if (!visit(V.sorted4[i])) break;
            for (int i = q0 - 1; i >= s0; --i) if (!visit(V.sorted4[i])) break;
        };
        auto scan_slab = [&](int bb) {
            const int s0 = V.slab_start[bb], s1 = V.slab_start[bb + 1];
            if (s0 >= s1) return;
            if (at >= s0 && at < s1) { scan_from(s0, s1, at); return; } /* the point's own slab: any split inside its window will do */
            int lo, hi;
            V.narrow(bb, s0, s1, p.y, lo, hi);
            scan_from(s0, s1, lower_bound_y(V, lo, hi, p.y));
        };
        const int b = slab_of(V.m, p.x); /* (inside [hb0, hb1): the point is indexed) */
        scan_slab(b);
        for (int bb = b + 1; bb < hb1; ++bb) {
            if (V.slab_start[bb] == V.slab_start[bb + 1]) continue;
            const float dx = V.slab_xmin[bb] - p.x;
            if (dx > 0.f && dx * dx > r2) break;
            scan_slab(bb);
        }
        for (int bb = b - 1; bb >= hb0; --bb) {
            if (V.slab_start[bb] == V.slab_start[bb + 1]) continue;
            const float dx = p.x - V.slab_xmax[bb];
            if (dx > 0.f && dx * dx > r2) break;
            scan_slab(bb);
        }
        smoothed[id] = (double)sum / (double)cnt * (1.0 / DEV_FIXED); /* (cnt >= 1: the point itself) */
    }
}

/* The accumulators of a tile: k_dev_target's words [0 .. 9] over the OWNED points -- except [3]: an owned point is indexed, so
   never DROPPED, and the word counts the evaluated halo points instead. */
#define DEVT_ACC_HALO 3
#define DEVT_ACC_WORDS DEV_ACC_BINS

/* k_dev_target for the positions [pos0, pos1), grid-stride: an owned matched point gets its target and enters the partial
   statistics; an evaluated halo point goes back to what k_devt_fill wrote -- its deviation has served the smoothing and is
   reported nowhere.  (Every other entry of a point that is not matched still holds the fill's value.)  Without smoothing v IS
   deviation: the two are not restrict.  The reduction is k_dev_target's: wave, workgroup, one integer atomic per word. */
__global__ void __launch_bounds__(DEV_T) k_devt_target(const float4 *__restrict__ sorted4, int pos0, int pos1, TileRange T,
        unsigned char *__restrict__ status, double *deviation, const double *v, const float *__restrict__ d2, int *__restrict__ ref_index,
        double allowance, double gain, double *__restrict__ target, unsigned long long *__restrict__ acc)
{
    __shared__ unsigned long long s_a[DEV_ACC_BINS];
    if (threadIdx.x < DEV_ACC_BINS) s_a[threadIdx.x] = 0;
    __syncthreads();
    unsigned long long cnt[4] = {0, 0, 0, 0}, proud = 0, below = 0, nlo = 0, hi = 0, fsum = 0, kd = 0;
    for (int pos = pos0 + blockIdx.x * DEV_T + threadIdx.x; pos < pos1; pos += gridDim.x * DEV_T) {
        const float4 p = sorted4[pos];
        if (!T.evaluated(p.x)) continue;
        const int i = idx_of(p);
        if (!T.owned(p.x)) {
            ++cnt[DEVT_ACC_HALO];
            status[i] = PPP_DEV_DROPPED; ref_index[i] = -1; deviation[i] = dev_nan();
            continue;
        }
        const int st = status[i];
        cnt[0] += st == PPP_DEV_MATCHED; cnt[1] += st == PPP_DEV_TOO_FAR; cnt[2] += st == PPP_DEV_NO_NORMAL;
        if (st != PPP_DEV_MATCHED) continue;
        const double x = v[i], over = x - allowance;
        target[i] = over > 0.0 ? gain * over : 0.0;
        proud += x > allowance; below += x < 0.0;
        nlo = max(nlo, ordered_key64(-x)); hi = max(hi, ordered_key64(x));
        fsum += (unsigned long long)llrint(x * DEV_FIXED);
        kd = max(kd, (unsigned long long)ordered_key(d2[i]));
    }
    for (int c = 0; c < 4; ++c) cnt[c] = wave_sum(cnt[c]);
    proud = wave_sum(proud); below = wave_sum(below); fsum = wave_sum(fsum);
    nlo = wave_max_bits(nlo); hi = wave_max_bits(hi); kd = wave_max_bits(kd);
    if ((threadIdx.x & 63) == 0) {
        for (int c = 0; c < 4; ++c) if (cnt[c]) atomicAdd(&s_a[DEV_ACC_STATUS + c], cnt[c]);
        if (cnt[0]) {
            atomicAdd(&s_a[DEV_ACC_PROUD], proud); atomicAdd(&s_a[DEV_ACC_BELOW], below); atomicAdd(&s_a[DEV_ACC_FIXSUM], fsum);
            atomicMax(&s_a[DEV_ACC_NMIN], nlo); atomicMax(&s_a[DEV_ACC_MAX], hi); atomicMax(&s_a[DEV_ACC_D2], kd);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int c = 0; c < 6; ++c) if (s_a[c]) atomicAdd(acc + c, s_a[c]);
        if (s_a[DEV_ACC_STATUS]) {
            atomicAdd(acc + DEV_ACC_FIXSUM, s_a[DEV_ACC_FIXSUM]);
            atomicMax(acc + DEV_ACC_NMIN, s_a[DEV_ACC_NMIN]); atomicMax(acc + DEV_ACC_MAX, s_a[DEV_ACC_MAX]); atomicMax(acc + DEV_ACC_D2, s_a[DEV_ACC_D2]);
        }
    }
}
