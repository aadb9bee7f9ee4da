/*
 * ppp_trimmed.h -- trimmed registration (ppp_register_trimmed): ppp_register's iteration in which
 * only the share `keep` of an evaluation's pairs with the smallest pair distance enters the 29 sums.  The cut is a rank
 * statistic over the pairs' float d2 read as 32-bit unsigned keys (a sum of squares: the keys order as the floats do), found
 * exactly by three counting passes over the key's digits -- 11, 11 and 10 bits, integer histograms, no order anywhere -- so
 * every output stays the same bits in every run.  An evaluation is k_trim_pair (the search, paid once: partner, key and the top
 * digit's histogram), k_trim_narrow<1> and <2> (the next two digits of the keys that share the prefix found so far),
 * k_trim_terms (the last digit's bin, the cut tau, and the sums over key <= tau) and ppp_registration.h's k_reg_step on those
 * sums.  Every workgroup finds the digit for itself in its prologue -- one scan of one histogram of at most 2 048 words --
 * so no launch stands between two passes; workgroup 0 leaves what it found for the next launch and for the host (TrimCut).
 * k_trim_scatter, once behind the chain, turns the last evaluation's keys into the status and d2 maps by cloud index.
 */
#pragma once
#include "ppp_registration.h"

#define TRIM_T 256
#define TRIM_B0 2048          /* key bits 31..21 */
#define TRIM_B1 2048          /* key bits 20..10 */
#define TRIM_B2 1024          /* key bits  9..0  */
#define TRIM_WORDS (TRIM_B0 + TRIM_B1 + TRIM_B2) /* one evaluation's three histograms */
#define TRIM_NONE 0xffffffffu /* the key of a query without a pair: above every float that is no NaN */
#define TRIM_NAN 0x7fc00000u  /* trim_d2 of an evaluation without a pair: the float quiet NaN, icp_nan()'s pattern narrowed */

/* what the passes of one evaluation leave for each other and for the host */
struct TrimCut {
    u32 paired, k;        /* the pairs the search found; the rank of the cut, 1-based (0: no pair) */
    u32 prefix1, rank1;   /* behind the top digit: the key's bits so far, the rank inside that bin */
    u32 prefix2, rank2;   /* behind the middle digit */
    u32 tau, pad;         /* the cut: the k-th smallest key; TRIM_NAN when paired == 0 */
};

/* B.78: k = ceil(keep * paired) in double, one product and one ceil, clamped to [1, paired]; 0 when there is no pair */
__host__ __device__ inline size_t trim_rank(double keep, size_t paired)
{
    if (!paired) return 0;
    const double c = ceil(keep * (double)paired);
    const size_t k = c >= 1.0 ? (size_t)c : (size_t)1;
    return k > paired ? paired : k;
}

/* Every thread of the workgroup: the bin of hist[0 .. PER * TRIM_T) that holds the rank-th smallest entry (1-based) and the rank
   inside that bin -> s_out[0], s_out[1]; the histogram's total -> s_out[2].  first: the rank is trim_rank(keep, total).  A thread
   owns PER neighbouring bins, one block scan orders the threads' sums, and the one thread whose range holds the rank walks its
   bins.  rank 0 (no pair) finds nothing: s_out[0] = s_out[1] = 0. */
template <int PER>
__device__ __forceinline__ void trim_select(const u32 *hist, bool first, double keep, u32 rank, int *s_scr, u32 *s_out)
{
    u32 c[PER];
    int sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) { c[i] = hist[threadIdx.x * PER + i]; sum += (int)c[i]; }
    int total;
    const int pre = block_exscan_w(sum, s_scr, &total);
    if (first) rank = (u32)trim_rank(keep, (size_t)total);
    if (threadIdx.x == 0) { s_out[0] = 0; s_out[1] = 0; s_out[2] = (u32)total; s_out[3] = rank; }
    __syncthreads();
    if (rank > (u32)pre && rank <= (u32)(pre + sum)) {
        u32 below = (u32)pre;
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            if (rank > below && rank <= below + c[i]) { s_out[0] = threadIdx.x * PER + i; s_out[1] = rank - below; }
            below += c[i];
        }
    }
    __syncthreads();
}

/* the workgroup's LDS histogram into the evaluation's: one 32-bit integer atomic per non-zero bin */
__device__ __forceinline__ void trim_flush(const u32 *s_h, int bins, u32 *__restrict__ hist)
{
    for (int b = threadIdx.x; b < bins; b += TRIM_T) {
        const u32 v = s_h[b];
        if (v) atomicAdd(hist + b, v);
    }
}

/* B.77: a thread per indexed point of the scan in slab order, grid-stride -- reg_terms_body's moved point (icp_move), query
   and pair rule (dev_pair).  A pair leaves the reference point it found (w: its cloud index) and its key; any other query the
   key TRIM_NONE.  The keys' top digits are counted in LDS and flushed once per workgroup. */
__global__ void __launch_bounds__(TRIM_T) k_trim_pair(const float4 *__restrict__ q4, int nq, const ContactIndex R, int nref, const IcpFrame F,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, float4 *__restrict__ partner, u32 *__restrict__ key, u32 *__restrict__ hist0)
{
    if (ctl->done) return;
    __shared__ u32 s_h[TRIM_B0];
    for (int b = threadIdx.x; b < TRIM_B0; b += TRIM_T) s_h[b] = 0;
    __syncthreads();
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        double m[3];
        icp_move(t, q4[at], m);
        const float qx = (float)m[0], qy = (float)m[1], qz = (float)m[2];
        u32 kk = TRIM_NONE;
        DevPair P;
        if (isfinite(qx) && isfinite(qy) && isfinite(qz) && dev_pair<true>(R, nref, 0, 0, qx, qy, qz, F.md2, P) == PPP_DEV_MATCHED) {
            kk = __float_as_uint(P.d2);
            partner[at] = P.q;
            atomicAdd(&s_h[kk >> 21], 1u);
        }
        key[at] = kk;
    }
    __syncthreads();
    trim_flush(s_h, TRIM_B0, hist0);
}

/* B.78, the middle digits: PASS 1 finds the top digit of the k-th smallest key in hist (the top digits' counts; their total is
   `paired`, so k comes from here) and counts bits 20..10 of the keys that carry it into next; PASS 2 finds the middle digit in
   hist (PASS 1's counts) at the rank PASS 1 left and counts bits 9..0 of the keys that carry both.  Over the stored keys: the
   search is not run again. */
template <int PASS>
__global__ void __launch_bounds__(TRIM_T) k_trim_narrow(const u32 *__restrict__ key, int nq, const IcpCtl *__restrict__ ctl, const u32 *hist,
        u32 *__restrict__ next, double keep, TrimCut *cut)
{
    if (ctl->done) return;
    constexpr int BINS = PASS == 1 ? TRIM_B1 : TRIM_B2;
    __shared__ u32 s_h[BINS];
    __shared__ int s_scr[16];
    __shared__ u32 s_out[4];
    if (PASS == 2 && cut->paired == 0) return;
    for (int b = threadIdx.x; b < BINS; b += TRIM_T) s_h[b] = 0;
    trim_select<(PASS == 1 ? TRIM_B0 : TRIM_B1) / TRIM_T>(hist, PASS == 1, keep, PASS == 1 ? 0u : cut->rank1, s_scr, s_out);
    const u32 prefix = PASS == 1 ? s_out[0] << 21 : cut->prefix1 | (s_out[0] << 10);
    const u32 mask = PASS == 1 ? 0xffe00000u : 0xfffffc00u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (PASS == 1) { cut->paired = s_out[2]; cut->k = s_out[3]; cut->prefix1 = prefix; cut->rank1 = s_out[1]; }
        else { cut->prefix2 = prefix; cut->rank2 = s_out[1]; }
    }
    if (s_out[2] == 0) return; /* no pair: nothing to count (PASS 1; PASS 2 left above) */
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        const u32 kk = key[at];
        if ((kk & mask) == prefix) atomicAdd(&s_h[PASS == 1 ? (kk >> 10) & (TRIM_B1 - 1) : kk & (TRIM_B2 - 1)], 1u);
    }
    __syncthreads();
    trim_flush(s_h, BINS, next);
}

/* B.78's last digit and B.79: tau from hist (PASS 2's counts) at the rank PASS 2 left, then reg_terms_body's 29 words
   (icp_add_terms) over the queries with key <= tau -- the moved point is made again from T (icp_move), the reference point and
   the key are read back -- and icp_flush.  acc[ICP_PAIRS] is `kept`. */
__global__ void __launch_bounds__(TRIM_T) k_trim_terms(const float4 *__restrict__ q4, int nq, const ContactIndex R, const IcpFrame F,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, const float4 *__restrict__ partner, const u32 *__restrict__ key,
        const u32 *hist, TrimCut *cut, unsigned long long *__restrict__ acc)
{
    if (ctl->done) return;
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
        double m[3];
        icp_move(t, q4[at], m);
        const float4 q = partner[at];
        icp_add_terms(a, m, q, R.normals4[idx_of(q)], F);
    }
    icp_flush<TRIM_T>(a, s_a, acc);
}

/* B.80: once behind the chain.  The keys are those of the last evaluation that ran -- evaluation ctl->steps, the one at the
   result -- and cuts[ctl->steps] holds its cut.  A thread per indexed point in slab order writes its own entries of the maps
   by cloud index; they hold DROPPED / NaN before the launch, which the points outside the index keep. */
__global__ void __launch_bounds__(TRIM_T) k_trim_scatter(const float4 *__restrict__ q4, int nq, const u32 *__restrict__ key, const IcpCtl *__restrict__ ctl,
        const TrimCut *__restrict__ cuts, int evals, int cap, unsigned char *__restrict__ status, float *__restrict__ d2)
{
    const int last = ctl->steps;
    if (last < 0 || last >= evals) return; /* the host reports the control words as corrupt */
    const u32 tau = cuts[last].tau;
    const bool none = cuts[last].paired == 0;
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        const int id = idx_of(q4[at]);
        if (id < 0 || id >= cap) continue;
        const u32 kk = key[at];
        if (kk == TRIM_NONE || none) { status[id] = PPP_TRIM_UNPAIRED; continue; }
        status[id] = kk <= tau ? PPP_TRIM_KEPT : PPP_TRIM_TRIMMED;
        d2[id] = __uint_as_float(kk);
    }
}
