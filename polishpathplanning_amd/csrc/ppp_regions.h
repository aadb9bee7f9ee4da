/*
 * ppp_regions.h -- connected regions of selected cloud points (ppp_get_regions): the step from a per-point
 * map of the contact queries (uncovered, overlap, narrow, or the caller's mask) to its connected components under "closer
 * than a link radius", each with its size, bounding box and centroid, and a label per point.
 *
 * Launches: k_reg_select (one thread per position of the slab index) -> the shared ordered compaction (ppp_preproc.h) to a
 * dense list of the selected positions -> k_reg_link (a concurrent union-find over the list: every pair within the radius is
 * united once, from its higher position) -> k_reg_flatten (every point's root; the per-region accumulators, aggregated in
 * the wave first) -> k_reg_labels (labels by cloud index, the totals) -> one more ordered compaction, over the labels: the
 * region rows in ascending label.  Everything after the select runs over the selected points only.
 *
 * The union-find lives in ORDINAL space: point k of the dense list, k ascending with the slab-index position, so neighbours
 * in space are near each other in the array (cloud order is a random permutation).  The larger root is always hooked under
 * the smaller one, so parent[k] <= k at every moment: paths descend strictly, no cycle can form whatever the interleaving,
 * and the root of a finished component is its smallest ordinal -- the same in every run.  Everything reduced per region is an
 * integer (count, ordered float keys, 64-bit fixed-point sums, the smallest cloud index), so the results are the same bits in
 * every run.  No float atomics.
 */
#pragma once
#include "ppp_contact.h"
#include "../../include/ppp_hip.h" /* PPP_REGIONS_* */

#define REG_T 256
/* No find / hook walk of a sound forest takes this many steps (each step descends at least one ordinal; halving keeps real
   paths to a handful): reaching it sets refusal bit 1 and ends the walk (PPP_ERR_CAPACITY on the host). */
#define REG_TRIPS (1 << 22)
#define REG_FIXED 1048576.0 /* 2^20: the centroid's fixed point (B.34) */

/* what a region accumulates, one per selected point (only a root's is used); the region rows are these, in label order */
struct RegAcc {
    int label;          /* the smallest cloud index */
    unsigned count;
    unsigned kmn[3];    /* ordered_key(-min): 0 = none */
    unsigned kmx[3];    /* ordered_key(max) */
    long long sum[3];   /* sum of llrint((double)p[c] * 2^20) */
};

/* what selects (ppp_get_regions' source): the map the source call left on the device, by cloud index */
struct RegSource {
    int kind;
    const unsigned char *bytes; /* UNCOVERED: the path coverage flags; MASK: the caller's bytes */
    const int *first, *last;    /* OVERLAP */
    const float *half_width;    /* NARROW */
    float threshold;
    __device__ inline bool selected(int id) const
    {
        switch (kind) {
        case PPP_REGIONS_UNCOVERED: return bytes[id] == 0;
        case PPP_REGIONS_OVERLAP: return last[id] > first[id];
        case PPP_REGIONS_NARROW: {
            const float a = fabsf(half_width[id]);
            return a <= 3.402823466e+38f && 2.f * a < threshold; /* as k_field_stats counts narrow */
        }
        default: return bytes[id] != 0;
        }
    }
};

/* One thread per position of the slab index (the indexed points: a non-finite point has no position and is never selected).
   A tile (ppp_get_regions_tile) selects inside its evaluated interval only: everything after the select runs over the list. */
__global__ void __launch_bounds__(REG_T) k_reg_select(const float4 *__restrict__ sorted4, int total, RegSource S, TileRange T,
        unsigned char *__restrict__ sel)
{
    const int pos = blockIdx.x * REG_T + threadIdx.x;
    if (pos >= total) return;
    const float4 p = sorted4[pos];
    sel[pos] = T.evaluated(p.x) && S.selected(idx_of(p)) ? 1 : 0;
}

/* the ordered compaction's selector: the selected positions, ascending, to list; ord[pos] = the point's ordinal (the -1 of the
   memset elsewhere); every selected point starts as its own region */
struct RegSel {
    using Val = unsigned char;
    const unsigned char *sel;
    int *list, *ord, *parent;
    RegAcc *acc;
    __device__ void begin() {}
    __device__ unsigned char load(int i) const { return sel[i]; }
    __device__ bool keep(int, unsigned char v) const { return v != 0; }
    __device__ void emit(int i, int k, unsigned char) const
    {
        list[k] = i; ord[i] = k; parent[k] = k;
        RegAcc a = {};
        a.label = 0x7fffffff;
        acc[k] = a;
    }
};

/* Parent words change under other workgroups' hands, and a CU's L1 is not coherent with another's: they are read and written
   with agent-scope relaxed atomics, never with plain loads. */
__device__ inline int reg_parent(const int *parent, int k) { return __hip_atomic_load(parent + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

/* the root of k, halving the path on the way (a halving write only ever replaces a parent by that parent's parent: parent[k]
   <= k stays true).  -1: REG_TRIPS steps (trips counts them across a caller's walks) */
__device__ inline int reg_find(int *parent, int k, int &trips)
{
    for (; trips < REG_TRIPS; ++trips) {
        const int p = reg_parent(parent, k);
        if (p == k) return k;
        const int g = reg_parent(parent, p);
        if (g == p) return p;
        atomicCAS(parent + k, p, g);
        k = g;
    }
    return -1;
}

/* a and b into one region: the larger root goes under the smaller by compare-and-swap; where another thread hooked it first,
   the walk goes on from what it found there.  false: REG_TRIPS steps */
__device__ inline bool reg_unite(int *parent, int a, int b, int &trips)
{
    for (; trips < REG_TRIPS; ++trips) {
        a = reg_find(parent, a, trips);
        b = reg_find(parent, b, trips);
        if (a < 0 || b < 0) return false;
        if (a == b) return true;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int was = atomicCAS(parent + hi, hi, lo);
        if (was == hi) return true;
        a = was; b = lo; /* hi is no root any more: was is above it */
    }
    return false;
}

/* A group of GRP lanes per selected point q (ordinal k, position pos): the y-windows of the slabs that [x - r, x + r] touches,
   found as the ball walk finds them (ball_slabs and its window, ppp_contact.h), cut off at pos: every selected candidate at a
   LOWER position with dist2_flann <= r2 is united with q, so each edge is met once.  The lanes of a group stride over a
   window's candidates; finds and hooks are each lane's own (lock-free).  err |= 1 where a walk reaches REG_TRIPS. */
template <int GRP>
__global__ void __launch_bounds__(REG_T) k_reg_link(const DevMeta *m, const float4 *__restrict__ sorted4, const int *__restrict__ slab_start,
        const int *__restrict__ ytab, const int *__restrict__ list, int nsel, const int *__restrict__ ord, int *parent, float r, float r2,
        int *__restrict__ err)
{
    const DynGrid G = dyn_grid(m);
    const int sub = threadIdx.x % GRP;
    const long long k = ((long long)blockIdx.x * REG_T + threadIdx.x) / GRP;
    if (k >= nsel) return;
    const int pos = list[k];
    const float4 q = sorted4[pos];
    const BallSlabs S = ball_slabs(G, q.x, q.y, r);
    int trips = 0;
    bool ok = true;
    for (int bb = S.blo; bb <= S.bhi && ok; ++bb) {
        const int s0 = slab_start[bb];
        if (s0 >= pos) break; /* this slab and those after it lie above q */
        int a, e;
        S.window(ytab, bb, s0, a, e);
        e = e < pos ? e : pos;
        for (int c = a + sub; c < e; c += GRP) {
            const int oc = ord[c];
            if (oc < 0) continue;
            const float4 p = sorted4[c];
            if (dist2_flann(q.x, q.y, q.z, p.x, p.y, p.z) <= r2 && !reg_unite(parent, (int)k, oc, trips)) { ok = false; break; }
        }
    }
    if (!ok) atomicOr(err, 1);
}

/* One thread per selected point, after every edge is in: its root (full compression: parent[k] = root) and its share of the
   root's accumulators -- the smallest cloud index (the label), the count, the box as ordered keys, the three fixed-point sums.
   Positions run in slab / y order, so most of a wave shares a root: the lanes that do vote with __ballot (as k_pcon_stats
   does), reduce among themselves and send ONE set of integer atomics; a lane alone with its root sends its own.  err |= 1
   where a walk reaches REG_TRIPS.  In a tile every listed point names the region (the label: halo points included), the
   points the tile owns (T.owned) alone count, span the box and enter the sums. */
__global__ void __launch_bounds__(REG_T) k_reg_flatten(const float4 *__restrict__ sorted4, const int *__restrict__ list, int nsel, int *parent,
        RegAcc *__restrict__ acc, TileRange T, int *__restrict__ err)
{
    const int k = blockIdx.x * REG_T + threadIdx.x; /* (whole waves go on: the votes below are the wave's) */
    const int lane = threadIdx.x & 63;
    bool have = k < nsel, own = false;
    int root = -1, id = 0x7fffffff;
    unsigned key[6] = {0, 0, 0, 0, 0, 0};
    long long fx[3] = {0, 0, 0};
    if (have) {
        root = k;
        int t = 0;
        for (; t < REG_TRIPS; ++t) {
            const int p = reg_parent(parent, root);
            if (p == root) break;
            root = p;
        }
        if (t >= REG_TRIPS) { atomicOr(err, 1); have = false; }
        else {
            __hip_atomic_store(parent + k, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float4 p = sorted4[list[k]];
            id = idx_of(p);
            const float c[3] = {p.x, p.y, p.z};
            own = T.owned(p.x);
            if (own)
                for (int i = 0; i < 3; ++i) {
                    key[i] = ordered_key(-c[i]); key[3 + i] = ordered_key(c[i]);
                    fx[i] = __double2ll_rn((double)c[i] * REG_FIXED);
                }
        }
    }
    u64 todo = __ballot(have);
    for (int it = 0; it < 64 && todo; ++it) { /* every turn serves its leading lane: at most 64 */
        const int lead = __ffsll((long long)todo) - 1;
        const int v = __shfl(root, lead, 64);
        const bool mine = have && root == v;
        const u64 same = __ballot(mine);
        todo &= ~same;
        int lab = id;
        unsigned cnt = own ? 1u : 0u, kk[6];
        long long ss[3];
        for (int i = 0; i < 6; ++i) kk[i] = key[i];
        for (int i = 0; i < 3; ++i) ss[i] = fx[i];
        if (__popcll(same) > 1) { /* (wave-uniform) */
            lab = mine ? id : 0x7fffffff;
            for (int o = 32; o > 0; o >>= 1) lab = min(lab, __shfl_xor(lab, o, 64));
            cnt = (unsigned)__popcll(__ballot(mine && own));
            for (int i = 0; i < 6; ++i) {
                unsigned x = mine ? key[i] : 0u;
                for (int o = 32; o > 0; o >>= 1) x = max(x, (unsigned)__shfl_xor((int)x, o, 64));
                kk[i] = x;
            }
            for (int i = 0; i < 3; ++i) ss[i] = wave_sum(mine ? fx[i] : 0ll);
        }
        if (lane == lead) {
            RegAcc *A = acc + v;
            atomicMin(&A->label, lab);
            atomicAdd(&A->count, cnt);
            for (int i = 0; i < 3; ++i) {
                atomicMax(&A->kmn[i], kk[i]); atomicMax(&A->kmx[i], kk[3 + i]);
                atomicAdd((unsigned long long *)&A->sum[i], (unsigned long long)ss[i]);
            }
        }
    }
}

/* One thread per selected point, after the accumulators are final: labels[cloud index] = its region's label; a root also
   records where its accumulators are (head_root[label], read by the region compaction) and counts into the totals --
   tot[0] regions, [1] regions of one point, [2] the largest count: wave sums, LDS, one atomic per workgroup. */
__global__ void __launch_bounds__(REG_T) k_reg_labels(const float4 *__restrict__ sorted4, const int *__restrict__ list, int nsel,
        const int *__restrict__ parent, const RegAcc *__restrict__ acc, int n, int *__restrict__ labels, int *__restrict__ head_root,
        unsigned *__restrict__ tot)
{
    __shared__ unsigned s_t[3];
    if (threadIdx.x < 3) s_t[threadIdx.x] = 0;
    __syncthreads();
    const int k = blockIdx.x * REG_T + threadIdx.x;
    int regions = 0, single = 0;
    unsigned largest = 0;
    if (k < nsel) {
        const int root = parent[k];
        const int lab = acc[root].label;
        labels[idx_of(sorted4[list[k]])] = lab;
        if (root == k && (unsigned)lab < (unsigned)n) { /* (a label is a cloud index of the region) */
            head_root[lab] = k;
            const unsigned c = acc[k].count;
            regions = 1; single = c == 1 ? 1 : 0; largest = c;
        }
    }
    regions = wave_sum(regions); single = wave_sum(single);
    for (int o = 32; o > 0; o >>= 1) largest = max(largest, (unsigned)__shfl_xor((int)largest, o, 64));
    if ((threadIdx.x & 63) == 0 && regions) { atomicAdd(&s_t[0], (unsigned)regions); atomicAdd(&s_t[1], (unsigned)single); atomicMax(&s_t[2], largest); }
    __syncthreads();
    if (threadIdx.x == 0 && s_t[0]) { atomicAdd(tot, s_t[0]); atomicAdd(tot + 1, s_t[1]); atomicMax(tot + 2, s_t[2]); }
}

/* the region rows in ascending label: cloud point i heads a region iff labels[i] == i; its row is its root's accumulators */
struct RegHeadSel {
    using Val = int;
    const int *labels, *head_root;
    const RegAcc *acc;
    RegAcc *rows;
    __device__ void begin() {}
    __device__ int load(int i) const { return labels[i]; }
    __device__ bool keep(int i, int v) const { return v == i; }
    __device__ void emit(int i, int k, int) const { rows[k] = acc[head_root[i]]; }
};
