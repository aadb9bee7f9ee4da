/*
 * ppp_robust.h -- robust registration (ppp_get_robust_registration_terms, ppp_register_robust):
 * ppp_register's iteration in which every pair enters the sums with Tukey's biweight of its point-to-plane residual r.  The
 * scale of the weight is the median of an evaluation's |r| -- a rank statistic over the floats (float)fabs(r) read as 32-bit
 * unsigned keys, found exactly by ppp_trimmed.h's three digit histograms at keep 0.5 -- so nothing has to choose a share of the
 * scan beforehand, and every output stays the same bits in every run.  An evaluation is k_rob_pair (the search, paid once:
 * partner, residual, key and the top digit's histogram), ppp_trimmed.h's k_trim_narrow<1> and <2> as they are, k_rob_terms (the
 * last digit's bin, the median tau, sigma, and the weighted sums) and ppp_registration.h's k_reg_step on those sums: word 0 of
 * an evaluation is `used`, the number of pairs with a weight above zero, which is what the step kernel reads as its pairs.
 * k_rob_scatter, once behind the chain, turns the last evaluation's residuals into the status, weight and residual maps by
 * cloud index.  rob_add_terms is a sibling of icp_add_terms, not a variant of it with the weight as an argument: k_reg_terms
 * and k_trim_terms keep their code, and with it their registers, untouched.
 */
#pragma once
#include "ppp_trimmed.h"

#define ROB_USED 0   /* the words of one evaluation: used, icp's A (21), b (6) and E at their places, the sum of the weights */
#define ROB_WSUM 29
#define ROB_WORDS 30
#define ROB_KEEP 0.5 /* the median: rank trim_rank(0.5, paired) */

/* what does not change along a robust chain beside IcpFrame */
struct RobScale { double tune, sigma_min; };

/* B.102: sigma = max(1.4826 m, sigma_min), m the double of the float with the bits of tau; the quiet NaN without a pair */
__host__ __device__ inline double rob_sigma(u32 tau, bool none, double sigma_min)
{
    if (none) return icp_nan();
    float mf; __builtin_memcpy(&mf, &tau, 4);
    const double s = 1.4826 * (double)mf;
    return s > sigma_min ? s : sigma_min;
}

/* B.103: Tukey's biweight of r at the cut cs = tune sigma: (1 - (r / cs)^2)^2 inside the cut, 0 from it on; tune = +INFINITY
   weighs every pair 1, cs == 0 the pairs with r == 0 only.  One rounding per written operation, no transcendental. */
__host__ __device__ inline double rob_weight(double r, double cs, double tune)
{
    if (tune == INFINITY) return 1.0;
    if (cs == 0.0) return r == 0.0 ? 1.0 : 0.0;
    const double u = r / cs;
    const double v = 1.0 - u * u;
    return fabs(u) < 1.0 ? v * v : 0.0;
}

/* B.69's residual of the moved point m against its partner q with the normal n */
__device__ __attribute__((always_inline)) inline double rob_residual(const double *m, const float4 &q, const float4 &n)
{
    const double ex = m[0] - (double)q.x, ey = m[1] - (double)q.y, ez = m[2] - (double)q.z;
    return ((ex * (double)n.x) + ey * (double)n.y) + ez * (double)n.z;
}

/* B.104: icp_add_terms's terms, each product times the weight w before it is rounded to 2^-shift: ((J_i J_k) w) 2^shift,
   ((J_i r) w) 2^shift, ((r r) w) 2^shift, and w 2^shift itself; a pair with w > 0 counts as used.  With w = 1 every word is
   icp_add_terms's. */
__device__ __attribute__((always_inline)) inline void rob_add_terms(unsigned long long *a, const double *m, double r, double w, const float4 &n,
                                                                   const IcpFrame &F)
{
    const double nx = (double)n.x, ny = (double)n.y, nz = (double)n.z;
    const double ux = (m[0] - F.c[0]) / F.Ln, uy = (m[1] - F.c[1]) / F.Ln, uz = (m[2] - F.c[2]) / F.Ln;
    const double J[6] = {uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx, nx, ny, nz};
    if (w > 0.0) a[ROB_USED] += 1;
    int at = ICP_A;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int k = i; k < 6; ++k, ++at) a[at] += (unsigned long long)llrint(((J[i] * J[k]) * w) * F.scale);
        a[ICP_B + i] += (unsigned long long)llrint(((J[i] * r) * w) * F.scale);
    }
    a[ICP_E] += (unsigned long long)llrint(((r * r) * w) * F.scale);
    a[ROB_WSUM] += (unsigned long long)llrint(w * F.scale);
}

/* icp_flush for ROB_WORDS words: over the wave, over the workgroup through LDS, one 64-bit integer atomic per non-zero word */
__device__ __attribute__((always_inline)) inline void rob_flush(unsigned long long *a, unsigned long long (*s_a)[ROB_WORDS],
                                                               unsigned long long *__restrict__ acc)
{
#pragma unroll
    for (int w = 0; w < ROB_WORDS; ++w) a[w] = wave_sum(a[w]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int w = 0; w < ROB_WORDS; ++w) s_a[threadIdx.x >> 6][w] = a[w];
    }
    __syncthreads();
    if (threadIdx.x < ROB_WORDS) {
        unsigned long long s = 0;
        for (int v = 0; v < TRIM_T / 64; ++v) s += s_a[v][threadIdx.x];
        if (s) atomicAdd(acc + threadIdx.x, s);
    }
}

/* B.101: k_trim_pair with the residual's key: a thread per indexed point of the scan in slab order, grid-stride -- the moved
   point (icp_move), the float query and the pair rule (dev_pair).  A pair leaves the reference point it found, its residual
   against that point's normal and the key of (float)fabs(r); any other query the key TRIM_NONE.  The keys' top digits are
   counted in LDS and flushed once per workgroup. */
__global__ void __launch_bounds__(TRIM_T) k_rob_pair(const float4 *__restrict__ q4, int nq, const ContactIndex R, int nref, const IcpFrame F,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, float4 *__restrict__ partner, double *__restrict__ res, u32 *__restrict__ key,
        u32 *__restrict__ hist0)
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
            const double r = rob_residual(m, P.q, P.n);
            kk = __float_as_uint((float)fabs(r));
            partner[at] = P.q;
            res[at] = r;
            atomicAdd(&s_h[kk >> 21], 1u);
        }
        key[at] = kk;
    }
    __syncthreads();
    trim_flush(s_h, TRIM_B0, hist0);
}

/* B.102's last digit and B.103, B.104: tau from hist (k_trim_narrow<2>'s counts) at the rank it left, sigma from tau, then the
   weighted words over every pair -- the moved point is made again from T (icp_move), the reference point and the residual are
   read back, the weight is rob_weight's -- and rob_flush.  Workgroup 0 leaves tau and sigma for the host and the scatter. */
__global__ void __launch_bounds__(TRIM_T) k_rob_terms(const float4 *__restrict__ q4, int nq, const ContactIndex R, const IcpFrame F, const RobScale S,
        const double *__restrict__ T, const IcpCtl *__restrict__ ctl, const float4 *__restrict__ partner, const double *__restrict__ res,
        const u32 *__restrict__ key, const u32 *hist, TrimCut *cut, double *sigma_out, unsigned long long *__restrict__ acc)
{
    if (ctl->done) return;
    __shared__ unsigned long long s_a[TRIM_T / 64][ROB_WORDS];
    __shared__ int s_scr[16];
    __shared__ u32 s_out[4];
    if (cut->paired == 0) {
        if (blockIdx.x == 0 && threadIdx.x == 0) { cut->tau = TRIM_NAN; *sigma_out = icp_nan(); }
        return;
    }
    trim_select<TRIM_B2 / TRIM_T>(hist, false, 0.0, cut->rank2, s_scr, s_out);
    const u32 tau = cut->prefix2 | s_out[0];
    const double sigma = rob_sigma(tau, false, S.sigma_min);
    const double cs = S.tune * sigma;
    if (blockIdx.x == 0 && threadIdx.x == 0) { cut->tau = tau; *sigma_out = sigma; }
    unsigned long long a[ROB_WORDS];
#pragma unroll
    for (int w = 0; w < ROB_WORDS; ++w) a[w] = 0;
    double t[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) t[i] = T[i];
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        if (key[at] == TRIM_NONE) continue;
        double m[3];
        icp_move(t, q4[at], m);
        const double r = res[at];
        rob_add_terms(a, m, r, rob_weight(r, cs, S.tune), R.normals4[idx_of(partner[at])], F);
    }
    rob_flush(a, s_a, acc);
}

/* the maps before the chain: DROPPED, the float quiet NaN and the double one in every entry (n >= 1) */
__global__ void __launch_bounds__(TRIM_T) k_rob_fill(int n, unsigned char *__restrict__ status, float *__restrict__ weight, double *__restrict__ residual)
{
    for (int i = blockIdx.x * TRIM_T + threadIdx.x; i < n; i += gridDim.x * TRIM_T) {
        status[i] = PPP_ROBUST_DROPPED;
        weight[i] = __uint_as_float(TRIM_NAN);
        residual[i] = icp_nan();
    }
}

/* B.105: once behind the chain.  The keys and the residuals are those of the last evaluation that ran -- evaluation
   ctl->steps, the one at the result -- and cuts[ctl->steps], sigma[ctl->steps] hold its scale.  A thread per indexed point in
   slab order writes its own entries of the maps by cloud index; they hold DROPPED / NaN before the launch, which the points
   outside the index keep. */
__global__ void __launch_bounds__(TRIM_T) k_rob_scatter(const float4 *__restrict__ q4, int nq, const u32 *__restrict__ key, const double *__restrict__ res,
        const IcpCtl *__restrict__ ctl, const TrimCut *__restrict__ cuts, const double *__restrict__ sigma, const RobScale S, int evals, int cap,
        unsigned char *__restrict__ status, float *__restrict__ weight, double *__restrict__ residual)
{
    const int last = ctl->steps;
    if (last < 0 || last >= evals) return; /* the host reports the control words as corrupt */
    const bool none = cuts[last].paired == 0;
    const double cs = S.tune * sigma[last];
    for (int at = blockIdx.x * TRIM_T + threadIdx.x; at < nq; at += gridDim.x * TRIM_T) {
        const int id = idx_of(q4[at]);
        if (id < 0 || id >= cap) continue;
        if (key[at] == TRIM_NONE || none) { status[id] = PPP_ROBUST_UNPAIRED; continue; }
        const double r = res[at];
        const double w = rob_weight(r, cs, S.tune);
        status[id] = w > 0.0 ? PPP_ROBUST_USED : PPP_ROBUST_REJECTED;
        weight[id] = (float)w;
        residual[id] = r;
    }
}
