/*
 * ppp_contact.hip -- the contact queries of the C ABI (include/ppp_hip.h) on a finished pass or a resident cloud: coverage,
 * path coverage, path contacts, path removal, the dwell schedule, the feed schedule, ppp_area2cloud, the principal curvatures,
 * the contact field and its tiles, the regions, their tiles and the merge.  The unit owns the kernels of ppp_contact.h,
 * ppp_regions.h, ppp_removal.h, ppp_dwell.h and ppp_feed.h; of the handle and the pass it sees what ppp_handle.h declares, and it
 * shares ppp_query_host.h with ppp_scan.hip, the unit of the calls that hold a scan against a reference cloud.  Compiled with
 * the engine's flags.
 */
#ifndef PPP_SINGLE_TU /* (a diagnostic build includes this file into the engine's unit) */
#define PPP_KERNELS_FOREIGN /* ppp_kernels.h, ppp_dynamic.h, ppp_compact.h: types and device helpers only -- their kernels are the engine's */
#endif
#include "ppp_query_host.h"
#include "ppp_regions.h"
#include "ppp_removal.h"
#include "ppp_dwell.h"
#include "ppp_feed.h"
#include <cstring>

extern "C" {

/* the kernels' view of the handle's knot tables, as they stand when the launch is made */
static KnotTable knot_table(const ppp_handle h)
{
    return KnotTable{h->node_x.p, h->node_y.p, h->node_z.p, h->node_start.p, h->node_cnt.p, h->node_cap};
}

/* What a pass did not build of what a contact query reads: the slab index (behind a window pass it keeps that pass's run
   state, gen_done with it, as every API mirror's does) and contact_buffers */
static int contact_prerequisites(ppp_handle h)
{
    int rc = index_ready(h, false);
    return rc ? rc : contact_buffers(h);
}

/* the opening of a query about the paths of a finished pass whose maps go by cloud index */
static int contact_query_begin(ppp_handle h, const char *what)
{
    int rc = ensure_ready(h, true, false);
    if (rc) return rc;
    rc = map_dev_err(h);
    if (rc) return rc;
    if (h->part_given)
        return fail(h, PPP_ERR_UNSUPPORTED, std::string(what) + ": the maps address the whole cloud: this handle holds a part (ppp_set_cloud_part)");
    return curvature_k_ok(h, h->P.curvature_k);
}

static PCovRange pcov_range(const ppp_handle h)
{
    return PCovRange{h->incl_lo, h->incl_hi, h->h_mn[0], h->h_mx[0], h->P.normal_radius, h->ranged ? 1 : 0};
}

/* the refusal word of the sample kernels: 1 wave_ball_leaves_range, 2 KnotTable::slice (or 2^24 samples on a slice), 4 the
   caps of k_pcon_offsets */
static int contact_refusal(ppp_handle h, const char *what, unsigned long long bits)
{
    const std::string w(what);
    if (bits & 2) return fail(h, PPP_ERR_HIP, w + ": a slice's knot table lies outside the node buffer");
    if (bits & 4) return fail(h, PPP_ERR_CAPACITY, w + ": more than 2^30 contact samples");
    if (bits & 1)
        return fail(h, PPP_ERR_CAPACITY, w + ": a contact search (Area2Cloud's neighbours, their normals or a ball) reaches beyond the indexed slice range: raise range_margin");
    return PPP_OK;
}

/* What both coverage calls share.  On the first question about a pass: the flags by cloud index (n16 uint4s: zero padding up to
   a multiple of 16 bytes) and the two result words zeroed, `mark` launches the balls (flags at C.flags.p, refusal word at
   C.count.p + 1), k_cov_count counts into C.count.p[0], one read brings both back.  Later questions answer from the result. */
static int flag_coverage(ppp_handle h, ppp_handle_s::FlagCoverage &C, const char *what, const std::function<int()> &mark, unsigned char *flags,
                         size_t cap, size_t *n, size_t *covered)
{
    const size_t N = h->n, n16 = (N + 15) / 16;
    if (C.serial != h->pass.serial()) {
        HIPCHK(h, C.flags.ensure(16 * std::max<size_t>(n16, 1))); HIPCHK(h, C.count.ensure(2));
        HIPCHK(h, hipMemsetAsync(C.flags.p, 0, 16 * std::max<size_t>(n16, 1), h->stream));
        HIPCHK(h, hipMemsetAsync(C.count.p, 0, 2 * sizeof(int), h->stream));
        int rc = mark();
        if (rc) return rc;
        if (n16)
            LAUNCH(h, "k_cov_count", k_cov_count, (unsigned)std::min<size_t>((n16 + COV_T - 1) / COV_T, 4 * (size_t)h->num_cus), COV_T, 0,
                   (const uint4 *)C.flags.p, (int)n16, C.count.p);
        int res[2] = {0, 0};
        HIPCHK(h, copy_sync(h, res, C.count.p, sizeof(res), hipMemcpyDeviceToHost));
        rc = contact_refusal(h, what, (unsigned)res[1]);
        if (rc) return rc;
        if (res[0] < 0 || (size_t)res[0] > N) return fail(h, PPP_ERR_HIP, std::string(what) + " count corrupt");
        C.covered = (size_t)res[0];
        C.serial = h->pass.serial();
    }
    if (n) *n = N;
    if (covered) *covered = C.covered;
    const size_t k = std::min(cap, N);
    if (flags && k) HIPCHK(h, copy_sync(h, flags, C.flags.p, k, hipMemcpyDeviceToHost));
    return PPP_OK;
}

int ppp_get_coverage(ppp_handle h, unsigned char *flags, size_t cap, size_t *n, size_t *covered)
{
    int rc = ensure_ready(h, true, false);
    if (rc) return rc;
    rc = map_dev_err(h);
    if (rc) return rc;
    if (h->P.walk != PPP_WALK_V1_CONTACT || !h->P.dynamic_adjustment || h->ranged || h->use_part || h->part_given)
        return fail(h, PPP_ERR_UNSUPPORTED, "coverage: only after a PPP_WALK_V1_CONTACT pass with dynamic_adjustment = 1 on a whole-cloud handle");
    auto balls = [h]() -> int { /* raw and adjusted paths of every slice, one launch */
        const int S = h->hmeta.S;
        if (S > 0)
            LAUNCH(h, "k_cov_balls", k_cov_balls, dim3((h->dyn_maxNB + DYN_WAVES - 1) / DYN_WAVES, S, 2), 64 * DYN_WAVES, 0, contact_index(h),
                   dyn_params(h), knot_table(h), h->dyn_raw_sc.p, h->dyn_maxNB, h->cov.flags.p);
        return PPP_OK;
    };
    return flag_coverage(h, h->cov, "coverage", balls, flags, cap, n, covered);
}

int ppp_get_path_coverage(ppp_handle h, unsigned char *flags, size_t cap, size_t *n, size_t *covered)
{
    int rc = contact_query_begin(h, "path coverage");
    if (rc) return rc;
    auto balls = [h]() -> int {
        int rc = contact_prerequisites(h);
        if (rc) return rc;
        const int S = h->hmeta.S, sb = std::min(h->sb, S), se = std::min(h->se, S);
        if (se <= sb) return PPP_OK;
        /* samples per slice of knots spanning the cloud's y range (the kernel strides past it where adjusted knots reach further) */
        const double yr = (double)h->h_mx[1] - (double)h->h_mn[1];
        const int nb = (int)std::min(65536.0, std::max(0.0, yr - 4) / (h->P.tool_radius / 4) + 4);
        for (int s0 = sb; s0 < se; s0 += 65535) /* (gridDim.y) */
            LAUNCH(h, "k_pcov_balls", k_pcov_balls, dim3((nb + DYN_WAVES - 1) / DYN_WAVES, std::min(se - s0, 65535)), 64 * DYN_WAVES, 0,
                   contact_index(h), dyn_params(h), knot_table(h), s0, pcov_range(h), h->pcov.flags.p, h->pcov.count.p + 1);
        return PPP_OK;
    };
    return flag_coverage(h, h->pcov, "path coverage", balls, flags, cap, n, covered);
}

/* The per-slice sample table of the last pass in h->pcon (off, tab, reach; k_pcon_offsets, k_pcon_samples), which the path
   contacts and the path removal both read: built on the first question about the pass, with what the pass left out
   (contact_prerequisites).  err: the device word the two kernels OR their refusals into, zeroed by the caller; the caller reads
   it back with its own results and only then calls pcon_table_accept, so a refused table is never reused. */
static int pcon_sample_table(ppp_handle h, const char *what, int *err)
{
    auto &C = h->pcon;
    if (C.tab_serial == h->pass.serial()) return PPP_OK;
    const int S = h->hmeta.S, sb = std::min(h->sb, S), se = std::min(h->se, S), nsl = std::max(se - sb, 0);
    int rc = contact_prerequisites(h);
    if (rc) return rc;
    C.tab_sb = sb; C.tab_nsl = nsl; C.tab_rows = 0;
    if (nsl <= 0) return PPP_OK;
    HIPCHK(h, C.off.ensure((size_t)nsl + 2));
    LAUNCH(h, "k_pcon_offsets", k_pcon_offsets, 1, PCON_T, 0, dyn_params(h), knot_table(h), sb, nsl, C.off.p, err);
    std::vector<int> off((size_t)nsl + 2);
    HIPCHK(h, copy_sync(h, off.data(), C.off.p, off.size() * sizeof(int), hipMemcpyDeviceToHost));
    rc = contact_refusal(h, what, (unsigned)off[nsl + 1]);
    if (rc) return rc;
    const int rows = off[nsl];
    int most = 0;
    for (int i = 0; i < nsl; ++i) most = std::max(most, off[i + 1] - off[i]);
    if (rows < 0 || most < 0) return fail(h, PPP_ERR_HIP, std::string(what) + ": sample table corrupt");
    if (rows > 0) {
        HIPCHK(h, C.tab.ensure((size_t)rows)); HIPCHK(h, C.reach.ensure(3 * (size_t)nsl));
        HIPCHK(h, hipMemsetAsync(C.reach.p, 0, 3 * (size_t)nsl * sizeof(unsigned), h->stream));
        const int gx = std::min((most + DYN_WAVES - 1) / DYN_WAVES, 16384);
        for (int s0 = 0; s0 < nsl; s0 += 65535) /* (gridDim.y) */
            LAUNCH(h, "k_pcon_samples", k_pcon_samples, dim3(gx, std::min(nsl - s0, 65535)), 64 * DYN_WAVES, 0, contact_index(h),
                   dyn_params(h), knot_table(h), C.off.p, sb, s0, pcov_range(h), C.tab.p, C.reach.p, err);
    }
    C.tab_rows = rows;
    return PPP_OK;
}
static void pcon_table_accept(ppp_handle h) { h->pcon.tab_serial = h->pass.serial(); }

int ppp_get_path_contacts(ppp_handle h, unsigned int *counts, int *first_slice, int *last_slice, size_t cap, ppp_contact_stats *stats)
{
    int rc = contact_query_begin(h, "path contacts");
    if (rc) return rc;
    const size_t N = h->n;
    auto &C = h->pcon;
    if (C.serial != h->pass.serial()) { /* first question about this pass */
        const size_t N1 = std::max<size_t>(N, 1);
        HIPCHK(h, C.counts.ensure(N1)); HIPCHK(h, C.first.ensure(N1)); HIPCHK(h, C.last.ensure(N1));
        HIPCHK(h, C.acc.ensure(70));
        HIPCHK(h, hipMemsetAsync(C.counts.p, 0, N1 * sizeof(unsigned), h->stream));
        HIPCHK(h, hipMemsetAsync(C.first.p, 0xff, N1 * sizeof(int), h->stream));
        HIPCHK(h, hipMemsetAsync(C.last.p, 0xff, N1 * sizeof(int), h->stream));
        HIPCHK(h, hipMemsetAsync(C.acc.p, 0, 70 * sizeof(unsigned long long), h->stream));
        int *err = (int *)(C.acc.p + 69);
        rc = pcon_sample_table(h, "path contacts", err);
        if (rc) return rc;
        if (C.tab_rows > 0) /* one thread per indexed point (at most N of them), PCON_T a round */
            LAUNCH(h, "k_pcon_points", k_pcon_points, (unsigned)std::min<size_t>((N + PCON_T - 1) / PCON_T, 1u << 20), PCON_T, 0,
                   h->meta.p, h->sorted4.p, C.tab.p, C.off.p, C.reach.p, C.tab_sb, C.tab_nsl, C.counts.p, C.first.p, C.last.p);
        LAUNCH(h, "k_pcon_stats", k_pcon_stats, (unsigned)std::min<size_t>((N1 + PCON_T - 1) / PCON_T, 2 * (size_t)h->num_cus), PCON_T, 0,
               C.counts.p, C.first.p, C.last.p, (int)N, err, C.acc.p);
        unsigned long long acc[69];
        HIPCHK(h, copy_sync(h, acc, C.acc.p, sizeof(acc), hipMemcpyDeviceToHost));
        rc = contact_refusal(h, "path contacts", acc[68]);
        if (rc) return rc;
        if (acc[64] > N || acc[65] > acc[64]) return fail(h, PPP_ERR_HIP, "path contacts: statistics corrupt");
        pcon_table_accept(h);
        ppp_contact_stats st = {};
        st.n = N; st.covered = (size_t)acc[64]; st.multi_slice = (size_t)acc[65];
        st.total = acc[66]; st.max_count = (unsigned)acc[67];
        st.hist[0] = N - st.covered;
        for (int b = 1; b < PPP_CONTACT_BINS; ++b) st.hist[b] = (size_t)acc[b];
        C.stats = st;
        C.serial = h->pass.serial();
    }
    if (stats) *stats = C.stats;
    const size_t k = std::min(cap, N);
    if (counts && k) HIPCHK(h, copy_sync(h, counts, C.counts.p, k * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (first_slice && k) HIPCHK(h, copy_sync(h, first_slice, C.first.p, k * sizeof(int), hipMemcpyDeviceToHost));
    if (last_slice && k) HIPCHK(h, copy_sync(h, last_slice, C.last.p, k * sizeof(int), hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* the double whose bit pattern an accumulator word holds (k_prem_range, k_dwell_stats, k_feed_stats) */
static double bits_as_double(unsigned long long k) { double d; memcpy(&d, &k, sizeof(d)); return d; }

static int removal_profile_ok(ppp_handle h, const char *what, int profile)
{
    if (profile != PPP_REMOVAL_FLAT && profile != PPP_REMOVAL_PARABOLIC && profile != PPP_REMOVAL_HERTZ)
        return fail(h, PPP_ERR_ARG, std::string(what) + ": unknown profile (PPP_REMOVAL_FLAT, _PARABOLIC or _HERTZ)");
    return PPP_OK;
}

/* a call that needs every slice of the walk on one handle refuses a slice-range handle */
static int whole_walk_only(ppp_handle h, const char *what, const char *why)
{
    if (h->P.slice_begin != 0 || h->P.slice_end != 0 || h->ranged || h->use_part) return fail(h, PPP_ERR_UNSUPPORTED, std::string(what) + ": " + why);
    return PPP_OK;
}

/* The point walk with the profile's weight over the handle's sample table: map[cloud index] = the sum of w * ds over the balls
   that hold the point, held flags beside it.  The one place that picks k_prem_points's instantiation. */
static int launch_prem_points(ppp_handle h, int profile, const double *ds, double *map)
{
    const auto &T = h->pcon;
    auto points = profile == PPP_REMOVAL_FLAT ? k_prem_points<PPP_REMOVAL_FLAT>
                : profile == PPP_REMOVAL_PARABOLIC ? k_prem_points<PPP_REMOVAL_PARABOLIC> : k_prem_points<PPP_REMOVAL_HERTZ>;
    LAUNCH(h, "k_prem_points", points, (unsigned)std::min<size_t>((h->n + PCON_T - 1) / PCON_T, 1u << 20), PCON_T, 0, h->meta.p, h->sorted4.p,
           T.tab.p, ds, T.off.p, T.reach.p, T.tab_nsl, map, h->prem.held.p);
    return PPP_OK;
}

/* the transposed walk of every row of the handle's sample table (k_dwell_back): num, and den where with_den.  The one place
   that picks k_dwell_back's instantiation. */
static int launch_dwell_back(ppp_handle h, int profile, bool with_den, const double *g, long long *num, long long *den)
{
    const auto &T = h->pcon;
    auto form = [with_den](auto with, auto without) { return with_den ? with : without; };
    auto back = profile == PPP_REMOVAL_FLAT ? form(k_dwell_back<PPP_REMOVAL_FLAT, true>, k_dwell_back<PPP_REMOVAL_FLAT, false>)
              : profile == PPP_REMOVAL_PARABOLIC ? form(k_dwell_back<PPP_REMOVAL_PARABOLIC, true>, k_dwell_back<PPP_REMOVAL_PARABOLIC, false>)
                                                 : form(k_dwell_back<PPP_REMOVAL_HERTZ, true>, k_dwell_back<PPP_REMOVAL_HERTZ, false>);
    LAUNCH(h, "k_dwell_back", back, (unsigned)((T.tab_rows + DYN_WAVES - 1) / DYN_WAVES), 64 * DYN_WAVES, 0, contact_index(h), T.tab.p, T.tab_rows, g,
           num, den);
    return PPP_OK;
}

/* The predicted removal: the sample table of the path contacts (shared with that call when the handle holds
   one for the pass), the path length of every sample (k_prem_ds, once per pass), the point walk with the profile's weight
   (k_prem_points) and the statistics in two phases (k_prem_range, k_prem_stats); kept per (pass, profile). */
int ppp_get_path_removal(ppp_handle h, int profile, double *removal, size_t cap, ppp_removal_stats *stats)
{
    int rc = contact_query_begin(h, "path removal");
    if (rc) return rc;
    rc = removal_profile_ok(h, "path removal", profile);
    if (rc) return rc;
    const size_t N = h->n;
    auto &R = h->prem;
    auto &M = R.slot[profile];
    const auto &T = h->pcon;
    if (M.serial != h->pass.serial()) { /* first question about this pass with this profile */
        const size_t N1 = std::max<size_t>(N, 1);
        const MapParts parts(h, N);
        const int grid = parts.grid, per = parts.per;
        HIPCHK(h, M.map.ensure(N1)); HIPCHK(h, R.held.ensure(N1));
        HIPCHK(h, R.acc.ensure(PREM_ACC_WORDS)); HIPCHK(h, R.psum.ensure(2 * (size_t)grid));
        HIPCHK(h, hipMemsetAsync(M.map.p, 0, N1 * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(R.held.p, 0, N1, h->stream));
        HIPCHK(h, hipMemsetAsync(R.acc.p, 0, PREM_ACC_WORDS * sizeof(unsigned long long), h->stream));
        rc = pcon_sample_table(h, "path removal", (int *)(R.acc.p + PREM_ACC_ERR));
        if (rc) return rc;
        const bool new_ds = R.ds_serial != h->pass.serial();
        if (T.tab_rows > 0) {
            if (new_ds) {
                HIPCHK(h, R.ds.ensure((size_t)T.tab_rows)); HIPCHK(h, R.slice_len.ensure((size_t)T.tab_nsl));
                LAUNCH(h, "k_prem_ds", k_prem_ds, (unsigned)T.tab_nsl, PCON_T, 0, T.tab.p, T.off.p, R.ds.p, R.slice_len.p);
            }
            rc = launch_prem_points(h, profile, R.ds.p, M.map.p);
            if (rc) return rc;
        }
        LAUNCH(h, "k_prem_range", k_prem_range, (unsigned)grid, PCON_T, 0, M.map.p, R.held.p, (int)N, R.acc.p);
        LAUNCH(h, "k_prem_stats", k_prem_stats, (unsigned)grid, PCON_T, 0, M.map.p, R.held.p, (int)N, per, R.acc.p, R.acc.p + PREM_ACC_BINS,
               R.psum.p, R.psum.p + grid);
        unsigned long long acc[PREM_ACC_WORDS];
        std::vector<double> psum(2 * (size_t)grid), len;
        HIPCHK(h, copy_sync(h, acc, R.acc.p, sizeof(acc), hipMemcpyDeviceToHost));
        rc = contact_refusal(h, "path removal", (unsigned)acc[PREM_ACC_ERR]);
        if (rc) return rc;
        if (acc[0] > N) return fail(h, PPP_ERR_HIP, "path removal: statistics corrupt");
        pcon_table_accept(h);
        HIPCHK(h, copy_sync(h, psum.data(), R.psum.p, psum.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (new_ds) { /* the slices' lengths in slice order */
            R.path_length = 0.0;
            if (T.tab_rows > 0) {
                len.resize((size_t)T.tab_nsl);
                HIPCHK(h, copy_sync(h, len.data(), R.slice_len.p, len.size() * sizeof(double), hipMemcpyDeviceToHost));
                for (double v : len) R.path_length += v;
            }
            R.ds_serial = h->pass.serial();
        }
        ppp_removal_stats st = {};
        st.n = N; st.touched = (size_t)acc[0];
        st.max_removal = st.touched ? bits_as_double(acc[1]) : (double)NAN; st.min_removal = st.touched ? bits_as_double(~acc[2]) : (double)NAN;
        for (int g = 0; g < grid; ++g) { st.sum += psum[(size_t)g]; st.sum_sq += psum[(size_t)grid + g]; }
        st.path_length = R.path_length;
        for (int b = 0; b < PPP_CONTACT_BINS; ++b) st.hist[b] = (size_t)acc[PREM_ACC_BINS + b];
        M.stats = st;
        M.serial = h->pass.serial();
    }
    if (stats) *stats = M.stats;
    const size_t k = std::min(cap, N);
    if (removal && k) HIPCHK(h, copy_sync(h, removal, M.map.p, k * sizeof(double), hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* The dwell schedule: the unit-feed map, the sample table, ds and the held flags come from
   ppp_get_path_removal's own call (built if the handle does not hold them, refused as it refuses); then every round's kernels
   back to back on the stream -- forward (k_dwell_scale + k_prem_points; the first round reads the unit-feed map, which IS the
   forward pass at t = 1), k_dwell_ratio, k_dwell_back, k_dwell_update -- the last forward pass, the residuals and the factors'
   statistics, and one wait.  Kept per (pass, profile, iterations, bounds) when there is no target. */
int ppp_get_path_dwell(ppp_handle h, int profile, const double *target, int iterations, double dwell_min, double dwell_max,
                       ppp_dwell_row *rows, size_t row_cap, double *removal, size_t cap, ppp_dwell_stats *stats)
{
    int rc = contact_query_begin(h, "path dwell");
    if (rc) return rc;
    rc = removal_profile_ok(h, "path dwell", profile);
    if (rc) return rc;
    if (iterations < 1 || iterations > 64) return fail(h, PPP_ERR_ARG, "path dwell: iterations must lie in [1, 64]");
    if (!(std::isfinite(dwell_min) && std::isfinite(dwell_max) && dwell_min > 0.0 && dwell_min <= 1.0 && dwell_max >= 1.0))
        return fail(h, PPP_ERR_ARG, "path dwell: the bounds must be finite with 0 < dwell_min <= 1 <= dwell_max");
    rc = whole_walk_only(h, "path dwell", "neighbouring slice ranges share the points of their overlap bands: a slice-range handle cannot solve alone");
    if (rc) return rc;
    const size_t N = h->n;
    auto &D = h->dwell;
    const bool reuse = !target && D.valid && D.serial == h->pass.serial() && D.profile == profile && D.iterations == iterations &&
                       D.dmin == dwell_min && D.dmax == dwell_max;
    if (!reuse) {
        D.valid = false;
        ppp_removal_stats rs = {};
        rc = ppp_get_path_removal(h, profile, nullptr, 0, &rs);
        if (rc) return rc;
        auto &R = h->prem;
        const auto &M = R.slot[profile];
        const auto &T = h->pcon;
        const int nrow = T.tab_rows, nsl = T.tab_nsl;
        const size_t N1 = std::max<size_t>(N, 1), R1 = (size_t)std::max(nrow, 1), touched = rs.touched;
        const MapParts parts(h, N);
        const int grid = parts.grid, per = parts.per;
        const unsigned gn = (unsigned)((N1 + PCON_T - 1) / PCON_T), gr = (unsigned)((R1 + PCON_T - 1) / PCON_T);
        HIPCHK(h, D.t.ensure(R1)); HIPCHK(h, D.dst.ensure(R1)); HIPCHK(h, D.num.ensure(R1)); HIPCHK(h, D.den.ensure(R1));
        HIPCHK(h, D.g.ensure(N1)); HIPCHK(h, D.map.ensure(N1)); HIPCHK(h, D.psum.ensure(2 * (size_t)grid));
        HIPCHK(h, D.acc.ensure(PREM_ACC_WORDS));
        double level = touched ? rs.sum / (double)touched : (double)NAN;
        const double *dtarget = nullptr;
        if (target) {
            if (touched) { /* the entries the solve reads */
                std::vector<unsigned char> held(N);
                HIPCHK(h, copy_sync(h, held.data(), R.held.p, N, hipMemcpyDeviceToHost));
                for (size_t i = 0; i < N; ++i)
                    if (held[i] && !(target[i] >= 0.0 && std::isfinite(target[i])))
                        return fail(h, PPP_ERR_ARG, "path dwell: the target must be finite and >= 0 at every touched point");
            }
            HIPCHK(h, D.target.ensure(N1));
            if (N) HIPCHK(h, copy_sync(h, D.target.p, target, N * sizeof(double), hipMemcpyHostToDevice));
            dtarget = D.target.p;
            if (touched) { /* L = the mean of T over the touched points, as k_prem_stats adds a map (its bins: all in bin 0, not read) */
                HIPCHK(h, hipMemsetAsync(D.acc.p, 0, PREM_ACC_WORDS * sizeof(unsigned long long), h->stream));
                LAUNCH(h, "k_prem_stats", k_prem_stats, (unsigned)grid, PCON_T, 0, D.target.p, R.held.p, (int)N, per, D.acc.p, D.acc.p + PREM_ACC_BINS,
                       D.psum.p, D.psum.p + grid);
                std::vector<double> ps((size_t)grid);
                HIPCHK(h, copy_sync(h, ps.data(), D.psum.p, ps.size() * sizeof(double), hipMemcpyDeviceToHost));
                double sum = 0.0;
                for (double v : ps) sum += v;
                level = sum / (double)touched;
            }
        }
        const bool walk = nrow > 0 && touched > 0, solve = walk && level > 0.0;
        HIPCHK(h, hipMemsetAsync(D.map.p, 0, N1 * sizeof(double), h->stream));
        HIPCHK(h, hipMemsetAsync(D.acc.p, 0, 4 * sizeof(unsigned long long), h->stream));
        std::vector<double> tv((size_t)nrow, 1.0), dsv((size_t)nrow);
        if (walk) {
            HIPCHK(h, hipMemsetAsync(D.g.p, 0, N1 * sizeof(double), h->stream));
            HIPCHK(h, copy_sync(h, D.t.p, tv.data(), tv.size() * sizeof(double), hipMemcpyHostToDevice));
            auto forward = [&]() -> int { /* D.map = the removal the factors predict */
                LAUNCH(h, "k_dwell_scale", k_dwell_scale, gr, PCON_T, 0, R.ds.p, D.t.p, nrow, D.dst.p);
                return launch_prem_points(h, profile, D.dst.p, D.map.p);
            };
            auto back = [&](bool with_den) { return launch_dwell_back(h, profile, with_den, D.g.p, D.num.p, D.den.p); };
            const double *cur = M.map.p; /* the forward pass at t = 1 */
            if (solve) LAUNCH(h, "k_dwell_resid", k_dwell_resid, (unsigned)grid, PCON_T, 0, cur, dtarget, level, R.held.p, (int)N, per, D.psum.p);
            for (int it = 0; solve && it < iterations; ++it) { /* no host wait in here */
                if (it > 0) { rc = forward(); if (rc) return rc; cur = D.map.p; }
                LAUNCH(h, "k_dwell_ratio", k_dwell_ratio, gn, PCON_T, 0, cur, dtarget, level, R.held.p, (int)N, D.g.p);
                rc = back(it == 0);
                if (rc) return rc;
                LAUNCH(h, "k_dwell_update", k_dwell_update, gr, PCON_T, 0, D.num.p, D.den.p, nrow, dwell_min, dwell_max, D.t.p);
            }
            if (!solve) { rc = back(true); if (rc) return rc; } /* den alone: which rows hold something */
            rc = forward();
            if (rc) return rc;
            if (solve) LAUNCH(h, "k_dwell_resid", k_dwell_resid, (unsigned)grid, PCON_T, 0, D.map.p, dtarget, level, R.held.p, (int)N, per, D.psum.p + grid);
            LAUNCH(h, "k_dwell_stats", k_dwell_stats, (unsigned)std::min<size_t>(gr, 2 * (size_t)h->num_cus), PCON_T, 0, D.t.p, D.den.p, nrow, dwell_min,
                   dwell_max, D.acc.p);
        }
        unsigned long long acc[4];
        std::vector<double> psum(2 * (size_t)grid, 0.0);
        HIPCHK(h, copy_sync(h, acc, D.acc.p, sizeof(acc), hipMemcpyDeviceToHost)); /* the one wait */
        if (solve) HIPCHK(h, copy_sync(h, psum.data(), D.psum.p, psum.size() * sizeof(double), hipMemcpyDeviceToHost));
        if (acc[0] > (size_t)nrow || acc[1] > (size_t)nrow) return fail(h, PPP_ERR_HIP, "path dwell: statistics corrupt");
        D.rows.assign((size_t)nrow, ppp_dwell_row{});
        double wsum = 0.0;
        if (nrow > 0) {
            std::vector<float4> tab((size_t)nrow);
            std::vector<int> off((size_t)nsl + 1);
            if (walk) HIPCHK(h, copy_sync(h, tv.data(), D.t.p, tv.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(h, copy_sync(h, dsv.data(), R.ds.p, dsv.size() * sizeof(double), hipMemcpyDeviceToHost));
            HIPCHK(h, copy_sync(h, tab.data(), T.tab.p, tab.size() * sizeof(float4), hipMemcpyDeviceToHost));
            HIPCHK(h, copy_sync(h, off.data(), T.off.p, off.size() * sizeof(int), hipMemcpyDeviceToHost));
            if (off[0] != 0 || off[(size_t)nsl] != nrow) return fail(h, PPP_ERR_HIP, "path dwell: sample table corrupt");
            for (int i = 0; i < nsl; ++i) {
                if (off[(size_t)i + 1] < off[(size_t)i]) return fail(h, PPP_ERR_HIP, "path dwell: sample table corrupt");
                double len = 0.0; /* the slice's scaled lengths in sample order, the slices in order: path_length's scheme */
                for (int j = off[(size_t)i]; j < off[(size_t)i + 1]; ++j) {
                    const float4 &q = tab[(size_t)j];
                    const double scaled = dsv[(size_t)j] * tv[(size_t)j];
                    len += scaled;
                    D.rows[(size_t)j] = ppp_dwell_row{T.tab_sb + i, q.x, q.y, q.z, std::sqrt(q.w), dsv[(size_t)j], tv[(size_t)j]};
                }
                wsum += len;
            }
        }
        ppp_dwell_stats st = {};
        st.n = N; st.touched = touched; st.rows = (size_t)nrow; st.at_min = (size_t)acc[0]; st.at_max = (size_t)acc[1];
        st.iterations = iterations; st.level = level;
        st.residual_before = st.residual_after = (double)NAN;
        if (solve) {
            double before = 0.0, after = 0.0;
            for (int g = 0; g < grid; ++g) { before += psum[(size_t)g]; after += psum[(size_t)grid + g]; }
            st.residual_before = std::sqrt(before / (double)touched); st.residual_after = std::sqrt(after / (double)touched);
        }
        st.max_dwell = acc[3] ? bits_as_double(acc[2]) : (double)NAN; st.min_dwell = acc[3] ? bits_as_double(~acc[3]) : (double)NAN;
        st.path_length = rs.path_length; st.time_factor = wsum / rs.path_length;
        D.stats = st;
        D.serial = h->pass.serial(); D.profile = profile; D.iterations = iterations; D.dmin = dwell_min; D.dmax = dwell_max;
        D.valid = !target;
    }
    if (stats) *stats = D.stats;
    const size_t kr = std::min(row_cap, D.rows.size()), k = std::min(cap, N);
    if (rows && kr) memcpy(rows, D.rows.data(), kr * sizeof(ppp_dwell_row));
    if (removal && k) HIPCHK(h, copy_sync(h, removal, D.map.p, k * sizeof(double), hipMemcpyDeviceToHost));
    return PPP_OK;
}

void ppp_default_feed_params(ppp_feed_params *fp)
{
    if (!fp) return;
    fp->feed = 20.0; fp->feed_max = 30.0; fp->accel = 100.0; fp->end_feed = 0.0; fp->link_feed = 100.0;
}

/* The feed schedule: the dwell rows come from ppp_get_path_dwell's own call (built if the handle does not hold
   them, refused as it refuses), the list from the last getPath (its stage list gathered into list order if a window pass left
   it in slots).  The kept slices' offsets into the list and into the rows are made on the host from the counts; then
   k_feed_map, k_feed_scan, k_feed_env, k_feed_time and its two followers and k_feed_stats back to back on the stream, and one
   wait.  Kept per (pass, profile, iterations, bounds, feed parameters) when there is no target. */
int ppp_get_path_feed(ppp_handle h, int profile, const double *target, int iterations, double dwell_min, double dwell_max,
                      const ppp_feed_params *fp, ppp_feed_row *rows, size_t cap, ppp_feed_stats *stats)
{
    int rc = contact_query_begin(h, "path feed");
    if (rc) return rc;
    if (!fp) return fail(h, PPP_ERR_ARG, "path feed: no feed parameters");
    if (!(std::isfinite(fp->feed) && fp->feed > 0.0)) return fail(h, PPP_ERR_ARG, "path feed: feed must be finite and > 0");
    if (!(std::isfinite(fp->feed_max) && fp->feed_max >= fp->feed)) return fail(h, PPP_ERR_ARG, "path feed: feed_max must be finite and >= feed");
    if (!(fp->accel > 0.0)) return fail(h, PPP_ERR_ARG, "path feed: accel must be > 0 (+INFINITY: no limit)");
    if (!std::isfinite(fp->end_feed)) return fail(h, PPP_ERR_ARG, "path feed: end_feed must be finite (< 0: no cap at a slice's ends)");
    if (!(std::isfinite(fp->link_feed) && fp->link_feed > 0.0)) return fail(h, PPP_ERR_ARG, "path feed: link_feed must be finite and > 0");
    rc = whole_walk_only(h, "path feed", "the dwell schedule it times cannot be solved on a slice-range handle");
    if (rc) return rc;
    if (h->aligned)
        return fail(h, PPP_ERR_UNSUPPORTED, "path feed: under ppp_trans2center the list's points are in the scanner's frame and the dwell rows in the aligned one");
    rc = ensure_ready(h, true, true); /* the waypoints must exist */
    if (rc) return rc;
    auto &F = h->feed;
    const ppp_feed_params P = *fp;
    const bool reuse = !target && F.valid && F.serial == h->pass.serial() && F.profile == profile && F.iterations == iterations &&
                       F.dmin == dwell_min && F.dmax == dwell_max && memcmp(&F.fp, &P, sizeof(P)) == 0;
    if (!reuse) {
        F.valid = false;
        ppp_dwell_stats dst = {};
        rc = ppp_get_path_dwell(h, profile, target, iterations, dwell_min, dwell_max, nullptr, 0, nullptr, 0, &dst);
        if (rc) return rc;
        const std::vector<ppp_dwell_row> &DR = h->dwell.rows;
        size_t Wl = 0, nkl = 0;
        rc = ppp_get_stage(h, PPP_STAGE_WP_XYZ, nullptr, 0, &Wl); /* the list order of wp_xyz */
        if (rc) return rc;
        rc = ppp_get_waypoint_counts(h, nullptr, 0, &nkl);
        if (rc) return rc;
        if (Wl > 0x7ffffff0u || nkl > 0x7ffffff0u) return fail(h, PPP_ERR_CAPACITY, "path feed: more than 2^31 waypoints");
        const int W = (int)Wl, nk = (int)nkl, first_kept = h->hmeta.first_kept;
        std::vector<int> off((size_t)nk + 1, 0), rowoff((size_t)nk + 1, 0);
        if (nk) { rc = ppp_get_waypoint_counts(h, off.data() + 1, nkl, &nkl); if (rc) return rc; }
        std::vector<int2> tiles;
        size_t slices = 0;
        for (int k = 0; k < nk; ++k) {
            const int m = off[(size_t)k + 1];
            if (m < 0 || m > W - off[(size_t)k]) return fail(h, PPP_ERR_HIP, "path feed: waypoint counts corrupt");
            off[(size_t)k + 1] = off[(size_t)k] + m;
            slices += m > 0;
            for (int i0 = 0; i0 < m; i0 += FEED_TILE) tiles.push_back(make_int2(k, i0));
        }
        if (off[(size_t)nk] != W) return fail(h, PPP_ERR_HIP, "path feed: waypoint counts corrupt");
        /* the rows come in (slice, sample) order: slice k's are those of walk slice first_kept + k */
        const size_t R = DR.size();
        std::vector<float> ry(R);
        std::vector<double> rt(R);
        {
            size_t j = 0;
            for (int k = 0; k < nk; ++k) {
                while (j < R && DR[j].slice < first_kept + k) ++j;
                rowoff[(size_t)k] = (int)j;
            }
            while (j < R && DR[j].slice < first_kept + nk) ++j;
            rowoff[(size_t)nk] = (int)j;
            for (j = 0; j < R; ++j) { ry[j] = DR[j].y; rt[j] = DR[j].dwell; }
        }
        F.host_rows.assign((size_t)W, ppp_feed_row{});
        unsigned long long acc[FEED_ACC_WORDS] = {};
        if (W > 0) {
            const size_t W1 = (size_t)W, K1 = (size_t)nk, R1 = std::max<size_t>(R, 1);
            HIPCHK(h, F.off.ensure(K1 + 1)); HIPCHK(h, F.rowoff.ensure(K1 + 1)); HIPCHK(h, F.tiles.ensure(tiles.size()));
            HIPCHK(h, F.ry.ensure(R1)); HIPCHK(h, F.rt.ensure(R1)); HIPCHK(h, F.cap.ensure(W1)); HIPCHK(h, F.D.ensure(W1));
            HIPCHK(h, F.tloc.ensure(W1)); HIPCHK(h, F.rec.ensure(W1)); HIPCHK(h, F.rows.ensure(W1)); HIPCHK(h, F.linkD.ensure(K1));
            HIPCHK(h, F.linkT.ensure(K1)); HIPCHK(h, F.slice_len.ensure(K1)); HIPCHK(h, F.slice_t.ensure(K1)); HIPCHK(h, F.acc.ensure(FEED_ACC_WORDS));
            HIPCHK(h, copy_sync(h, F.off.p, off.data(), (K1 + 1) * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(h, copy_sync(h, F.rowoff.p, rowoff.data(), (K1 + 1) * sizeof(int), hipMemcpyHostToDevice));
            HIPCHK(h, copy_sync(h, F.tiles.p, tiles.data(), tiles.size() * sizeof(int2), hipMemcpyHostToDevice));
            if (R) {
                HIPCHK(h, copy_sync(h, F.ry.p, ry.data(), R * sizeof(float), hipMemcpyHostToDevice));
                HIPCHK(h, copy_sync(h, F.rt.p, rt.data(), R * sizeof(double), hipMemcpyHostToDevice));
            }
            HIPCHK(h, hipMemsetAsync(F.linkD.p, 0, K1 * sizeof(long long), h->stream));
            HIPCHK(h, hipMemsetAsync(F.linkT.p, 0, K1 * sizeof(long long), h->stream));
            HIPCHK(h, hipMemsetAsync(F.acc.p, 0, FEED_ACC_WORDS * sizeof(unsigned long long), h->stream));
            const unsigned gw = (unsigned)((W1 + PCON_T - 1) / PCON_T);
            LAUNCH(h, "k_feed_map", k_feed_map, gw, PCON_T, 0, h->wp_xyz.p, F.off.p, nk, W, first_kept, F.rowoff.p, F.ry.p, F.rt.p, P.feed, P.feed_max,
                   P.end_feed, P.link_feed, F.rows.p, F.cap.p, F.D.p, F.linkD.p, F.linkT.p);
            LAUNCH(h, "k_feed_scan", k_feed_scan, (unsigned)nk, PCON_T, 0, F.off.p, F.D.p, F.cap.p, F.rec.p, F.slice_len.p);
            LAUNCH(h, "k_feed_env", k_feed_env, (unsigned)tiles.size(), FEED_TILE, 0, F.tiles.p, F.off.p, F.rec.p, P.accel, F.rows.p);
            LAUNCH(h, "k_feed_time", k_feed_time, (unsigned)nk, PCON_T, 0, F.off.p, F.rows.p, F.D.p, F.linkT.p, P.accel, F.tloc.p, F.slice_t.p);
            LAUNCH(h, "k_feed_time_slices", k_feed_time_slices, 1, PCON_T, 0, nk, F.slice_t.p, F.linkT.p, F.slice_len.p, F.linkD.p, F.acc.p);
            LAUNCH(h, "k_feed_time_rows", k_feed_time_rows, gw, PCON_T, 0, W, first_kept, F.tloc.p, F.slice_t.p, F.rows.p);
            LAUNCH(h, "k_feed_stats", k_feed_stats, std::min<unsigned>(gw, 2u * (unsigned)h->num_cus), PCON_T, 0, F.rows.p, W, F.acc.p);
            HIPCHK(h, copy_sync(h, acc, F.acc.p, sizeof(acc), hipMemcpyDeviceToHost)); /* the one wait */
            HIPCHK(h, copy_sync(h, F.host_rows.data(), F.rows.p, W1 * sizeof(ppp_feed_row), hipMemcpyDeviceToHost));
            if (acc[0] + acc[1] + acc[2] + acc[3] != (unsigned long long)W) return fail(h, PPP_ERR_HIP, "path feed: statistics corrupt");
        }
        auto fixed = [](unsigned long long k, double one) { return (double)(long long)k * (1.0 / one); };
        ppp_feed_stats st = {};
        st.W = (size_t)W; st.slices = slices;
        st.by_dwell = (size_t)acc[FEED_ACC_LIMIT]; st.by_feed_max = (size_t)acc[FEED_ACC_LIMIT + 1]; st.by_end = (size_t)acc[FEED_ACC_LIMIT + 2];
        st.by_accel = (size_t)acc[FEED_ACC_LIMIT + 3];
        st.max_feed = W ? bits_as_double(acc[FEED_ACC_MAX]) : (double)NAN; st.min_feed = W ? bits_as_double(~acc[FEED_ACC_NMIN]) : (double)NAN;
        st.path_length = fixed(acc[FEED_ACC_PATH], FEED_LEN_FIXED); st.link_length = fixed(acc[FEED_ACC_LINK], FEED_LEN_FIXED);
        st.duration = fixed(acc[FEED_ACC_DUR], FEED_TIME_FIXED); st.duration_links = fixed(acc[FEED_ACC_DUR_LINKS], FEED_TIME_FIXED);
        st.duration_nominal = st.path_length / P.feed;
        F.stats = st;
        F.serial = h->pass.serial(); F.profile = profile; F.iterations = iterations; F.dmin = dwell_min; F.dmax = dwell_max; F.fp = P;
        F.valid = !target;
    }
    if (stats) *stats = F.stats;
    const size_t k = std::min(cap, F.host_rows.size());
    if (rows && k) memcpy(rows, F.host_rows.data(), k * sizeof(ppp_feed_row));
    return PPP_OK;
}

int ppp_area2cloud(ppp_handle h, const double *pts_xyz, size_t k, int key, float *out3)
{
    int rc = index_ready(h, false); /* complete index: slabs beyond the LDS capacity go through the arena pass first */
    if (rc) return rc;
    if (!k) return PPP_OK;
    if (!pts_xyz || !out3 || (key != 0 && key != 1)) return fail(h, PPP_ERR_ARG, "bad arguments");
    if (int rck = curvature_k_ok(h, h->P.curvature_k)) return rck;
    rc = ensure_dynamic_buffers(h);
    if (rc) return rc;
    rc = enqueue_normals(h);
    if (rc) return rc;
    HIPCHK(h, h->scratch.ensure(k * 36 + 64));
    double *dq = (double *)h->scratch.p;
    float *dout = (float *)(dq + 3 * k);
    HIPCHK(h, hipMemcpyAsync(dq, pts_xyz, k * 24, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "k_area2cloud_api", k_area2cloud_api, (unsigned)((k + DYN_WAVES - 1) / DYN_WAVES), 64 * DYN_WAVES, 0, contact_index(h), dyn_params(h),
           dq, (int)k, key, dout);
    HIPCHK(h, hipMemcpyAsync(out3, dout, k * 12, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PPP_OK;
}

int ppp_principal_curvatures_at(ppp_handle h, const float *q_xyz, size_t k, float *out5)
{
    int rc = index_ready(h, false); /* complete index: slabs beyond the LDS capacity go through the arena pass first */
    if (rc) return rc;
    if (!k) return PPP_OK;
    if (!q_xyz || !out5 || k > 0x7fffffffu / 8) return fail(h, PPP_ERR_ARG, "bad arguments");
    if (int rck = curvature_k_ok(h, h->P.curvature_k)) return rck;
    rc = contact_buffers(h);
    if (rc) return rc;
    HIPCHK(h, h->scratch.ensure(k * 32 + 64));
    float *dq = (float *)h->scratch.p, *dout = dq + 3 * k;
    HIPCHK(h, hipMemcpyAsync(dq, q_xyz, k * 12, hipMemcpyHostToDevice, h->stream));
    LAUNCH(h, "k_field_waves", k_field_waves, (unsigned)((k + DYN_WAVES - 1) / DYN_WAVES), 64 * DYN_WAVES, 0, contact_index(h), dyn_params(h),
           dq, (int)k, dout, (float *)nullptr);
    HIPCHK(h, hipMemcpyAsync(out5, dout, k * 20, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PPP_OK;
}

/* the opening of the field and region calls: a handle, on its device, that holds a cloud and holds all of it.  what: the call's
   name in the refusal, why: what a part cannot give it */
static int whole_cloud_begin(ppp_handle h, const char *what, const char *why)
{
    if (!h) return PPP_ERR_ARG;
    HIPCHK(h, hipSetDevice(h->device));
    if (!h->have_cloud) return fail(h, PPP_ERR_ARG, "no cloud set");
    if (h->part_given) return fail(h, PPP_ERR_UNSUPPORTED, std::string(what) + ": " + why + ": this handle holds a part (ppp_set_cloud_part)");
    return PPP_OK;
}

/* the parameters a contact field depends on */
static bool same_contact_params(const ppp_params &P, const ppp_params &F)
{
    return P.tool_radius == F.tool_radius && P.depth == F.depth && P.toolthickness == F.toolthickness && P.curvature_k == F.curvature_k &&
           P.normal_radius == F.normal_radius && P.change_range == F.change_range;
}

/* the statistics of a stored half-width map for one min_width (k_field_stats): hw = N half widths by cloud index */
static int field_statistics(ppp_handle h, const float *hw, DevBuf<unsigned long long> &dacc, DevBuf<double> &dpsum, float min_width,
                            ppp_contact_field_stats &st)
{
    const size_t N = h->n;
    const MapParts parts(h, N);
    const int grid = parts.grid, per = parts.per;
    HIPCHK(h, dacc.ensure(68)); HIPCHK(h, dpsum.ensure((size_t)grid));
    HIPCHK(h, hipMemsetAsync(dacc.p, 0, 68 * sizeof(unsigned long long), h->stream));
    LAUNCH(h, "k_field_stats", k_field_stats, (unsigned)grid, PCON_T, 0, hw, (int)N, per, h->P.tool_radius, min_width, dacc.p, dpsum.p);
    unsigned long long acc[68];
    std::vector<double> psum((size_t)grid);
    HIPCHK(h, copy_sync(h, acc, dacc.p, sizeof(acc), hipMemcpyDeviceToHost));
    HIPCHK(h, copy_sync(h, psum.data(), dpsum.p, psum.size() * sizeof(double), hipMemcpyDeviceToHost));
    if (acc[64] > N || acc[65] > acc[64]) return fail(h, PPP_ERR_HIP, "contact field: statistics corrupt");
    st = {};
    st.n = N; st.valid = (size_t)acc[64]; st.narrow = (size_t)acc[65];
    st.min_abs_r = st.valid ? -ordered_unkey((unsigned)acc[66]) : NAN; st.max_abs_r = st.valid ? ordered_unkey((unsigned)acc[67]) : NAN;
    for (double v : psum) st.sum_abs_r += v;
    for (int b = 0; b < PPP_CONTACT_BINS; ++b) st.hist[b] = (size_t)acc[b];
    return PPP_OK;
}
static int field_statistics(ppp_handle h, float min_width)
{
    auto &C = h->field;
    int rc = field_statistics(h, C.hw.p, C.acc, C.psum, min_width, C.stats);
    if (!rc) C.min_width = min_width;
    return rc;
}

int ppp_get_contact_field(ppp_handle h, float *curv5, float *half_width, size_t cap, float min_width, ppp_contact_field_stats *stats)
{
    if (int rcb = whole_cloud_begin(h, "contact field", "the maps address the whole cloud")) return rcb;
    if (h->P.slice_begin != 0 || h->P.slice_end != 0)
        return fail(h, PPP_ERR_UNSUPPORTED, "contact field: a slice-range handle indexes a part of the cloud only");
    if (int rck = curvature_k_ok(h, h->P.curvature_k)) return rck;
    if (!(min_width > 0.f)) min_width = 0.f;
    const size_t N = h->n;
    auto &C = h->field;
    const ppp_params &P = h->P, &F = C.P;
    const bool same = C.valid && same_contact_params(P, F);
    if (!same) {
        C.valid = false;
        int rc = index_ready(h, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
        if (rc) return rc;
        if (h->ranged || h->use_part) return fail(h, PPP_ERR_UNSUPPORTED, "contact field: a slice-range handle indexes a part of the cloud only");
        rc = contact_buffers(h);
        if (rc) return rc;
        const size_t N1 = std::max<size_t>(N, 1);
        HIPCHK(h, C.curv.ensure(5 * N1)); HIPCHK(h, C.hw.ensure(N1));
        HIPCHK(h, hipMemsetAsync(C.curv.p, 0xff, 5 * N1 * sizeof(float), h->stream)); /* dropped points: NaN */
        HIPCHK(h, hipMemsetAsync(C.hw.p, 0xff, N1 * sizeof(float), h->stream));
        const int nsorted = h->hmeta.n_sorted;
        if (nsorted < 0 || (size_t)nsorted > N) return fail(h, PPP_ERR_HIP, "contact field: index corrupt");
        if (nsorted > 0) /* a wave per FIELD_Q indexed points, in slab / y order */
            LAUNCH(h, "k_field_batch", k_field_batch, (unsigned)((nsorted + FIELD_Q * DYN_WAVES - 1) / (FIELD_Q * DYN_WAVES)), 64 * DYN_WAVES, 0,
                   contact_index(h), dyn_params(h), nsorted, C.curv.p, C.hw.p);
        rc = field_statistics(h, min_width);
        if (rc) return rc;
        C.P = h->P;
        C.valid = true; ++C.built;
    } else if (stats && min_width != C.min_width) {
        int rc = field_statistics(h, min_width);
        if (rc) return rc;
    }
    if (stats) *stats = C.stats;
    const size_t k = std::min(cap, N);
    if (curv5 && k) HIPCHK(h, copy_sync(h, curv5, C.curv.p, 5 * k * sizeof(float), hipMemcpyDeviceToHost));
    if (half_width && k) HIPCHK(h, copy_sync(h, half_width, C.hw.p, k * sizeof(float), hipMemcpyDeviceToHost));
    return PPP_OK;
}

static void tile_field_stats(ppp_contact_field_tile_stats &o, const ppp_contact_field_stats &st)
{
    o.n = st.n; o.valid = st.valid; o.narrow = st.narrow; o.min_abs_r = st.min_abs_r; o.max_abs_r = st.max_abs_r; o.sum_abs_r = st.sum_abs_r;
    memcpy(o.hist, st.hist, sizeof(o.hist));
}

int ppp_get_contact_field_tile(ppp_handle h, float *curv5, float *half_width, unsigned char *owned, size_t cap, float halo,
                               float min_width, ppp_contact_field_tile_stats *stats)
{
    if (int rcb = whole_cloud_begin(h, "contact field tile", "the maps address the whole cloud")) return rcb;
    if (int rck = curvature_k_ok(h, h->P.curvature_k)) return rck;
    if (!(halo >= 0.f && halo <= 3.402823466e+38f)) return fail(h, PPP_ERR_ARG, "contact field tile: halo must be a finite number >= 0");
    if (!(min_width > 0.f)) min_width = 0.f;
    const size_t N = h->n;
    auto &C = h->ftile;
    const ppp_params &P = h->P, &F = C.P;
    const bool same = C.valid && same_contact_params(P, F) && P.walk == F.walk && P.slice_begin == F.slice_begin && P.slice_end == F.slice_end &&
                      P.range_margin == F.range_margin && halo == C.halo;
    if (!same) {
        C.valid = false;
        int rc = index_ready(h, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
        if (rc) return rc;
        rc = contact_buffers(h);
        if (rc) return rc;
        TileRange T;
        rc = tile_range(h, halo, T);
        if (rc) return rc;
        int pos0, pos1;
        rc = tile_positions(h, T, pos0, pos1);
        if (rc) return rc;
        const size_t N1 = std::max<size_t>(N, 1);
        HIPCHK(h, C.curv.ensure(5 * N1)); HIPCHK(h, C.hw.ensure(N1)); HIPCHK(h, C.hw_own.ensure(N1)); HIPCHK(h, C.owned.ensure(N1));
        HIPCHK(h, C.cnt.ensure(4));
        HIPCHK(h, hipMemsetAsync(C.curv.p, 0xff, 5 * N1 * sizeof(float), h->stream)); /* not evaluated: NaN */
        HIPCHK(h, hipMemsetAsync(C.hw.p, 0xff, N1 * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(C.hw_own.p, 0xff, N1 * sizeof(float), h->stream));
        HIPCHK(h, hipMemsetAsync(C.owned.p, 0, N1, h->stream));
        HIPCHK(h, hipMemsetAsync(C.cnt.p, 0, 4 * sizeof(int), h->stream));
        if (pos1 > pos0) {
            const int np = pos1 - pos0;
            LAUNCH(h, "k_tile_mark", k_tile_mark, (unsigned)((np + PCON_T - 1) / PCON_T), PCON_T, 0, h->sorted4.p, pos0, pos1, T, C.owned.p, C.cnt.p);
            LAUNCH(h, "k_field_tile", k_field_tile, (unsigned)((np + FIELD_Q * DYN_WAVES - 1) / (FIELD_Q * DYN_WAVES)), 64 * DYN_WAVES, 0,
                   contact_index(h), dyn_params(h), pos0, pos1, T, pcov_range(h), C.curv.p, C.hw.p, C.hw_own.p, C.cnt.p + 2);
        }
        int cnt[3];
        HIPCHK(h, copy_sync(h, cnt, C.cnt.p, sizeof(cnt), hipMemcpyDeviceToHost));
        if (cnt[2])
            return fail(h, PPP_ERR_CAPACITY, "contact field tile: a search of an evaluated point (its neighbours or their normals) reaches beyond the indexed slice range: raise range_margin");
        if (cnt[0] < 0 || cnt[1] < cnt[0] || (size_t)cnt[1] > N) return fail(h, PPP_ERR_HIP, "contact field tile: counts corrupt");
        ppp_contact_field_stats st;
        rc = field_statistics(h, C.hw_own.p, C.acc, C.psum, min_width, st);
        if (rc) return rc;
        C.stats = {};
        C.stats.owned = (size_t)cnt[0]; C.stats.evaluated = (size_t)cnt[1]; C.stats.own_lo = T.own_lo; C.stats.own_hi = T.own_hi;
        tile_field_stats(C.stats, st);
        C.P = h->P; C.halo = halo; C.min_width = min_width;
        C.valid = true; ++C.built;
    } else if (stats && min_width != C.min_width) {
        ppp_contact_field_stats st;
        int rc = field_statistics(h, C.hw_own.p, C.acc, C.psum, min_width, st);
        if (rc) return rc;
        tile_field_stats(C.stats, st);
        C.min_width = min_width;
    }
    if (stats) *stats = C.stats;
    const size_t k = std::min(cap, N);
    if (curv5 && k) HIPCHK(h, copy_sync(h, curv5, C.curv.p, 5 * k * sizeof(float), hipMemcpyDeviceToHost));
    if (half_width && k) HIPCHK(h, copy_sync(h, half_width, C.hw.p, k * sizeof(float), hipMemcpyDeviceToHost));
    if (owned && k) HIPCHK(h, copy_sync(h, owned, C.owned.p, k, hipMemcpyDeviceToHost));
    return PPP_OK;
}

/* lanes per selected point in k_reg_link */
#ifndef REG_GROUP
#define REG_GROUP 8
#endif

/* The device work of a region call, behind index_ready and the source's own call: select inside T's evaluated interval, list,
   link, flatten (T's owned points count), label, the rows in ascending label -- into h->regions' buffers.  half_width: the map
   PPP_REGIONS_NARROW reads.  nsel / nreg: the listed points and the regions (a tile's: every component of the list). */
static int regions_compute(ppp_handle h, int source, const unsigned char *mask, const float *half_width, float threshold, float link,
                           const TileRange &T, size_t &nsel, size_t &nreg, unsigned tot[4])
{
    const size_t N = h->n;
    auto &R = h->regions;
    R.valid = false;
    nsel = nreg = 0;
    const int ns = h->hmeta.n_sorted;
    if (ns < 0 || (size_t)ns > N || N > 0x7fffffffu) return fail(h, PPP_ERR_HIP, "regions: index corrupt");
    const size_t N1 = std::max<size_t>(N, 1);
    const int nb_sel = (ns + COMPACT_CHUNK - 1) / COMPACT_CHUNK, nb_head = (int)((N + COMPACT_CHUNK - 1) / COMPACT_CHUNK);
    HIPCHK(h, R.labels.ensure(N1)); HIPCHK(h, R.head_root.ensure(N1)); HIPCHK(h, R.tot.ensure(8));
    HIPCHK(h, R.cnt.ensure((size_t)std::max(nb_sel, nb_head) + 1));
    HIPCHK(h, hipMemsetAsync(R.labels.p, 0xff, N1 * sizeof(int), h->stream)); /* not selected: -1 */
    HIPCHK(h, hipMemsetAsync(R.tot.p, 0, 8 * sizeof(unsigned), h->stream));
    int *err = (int *)R.tot.p + 3;
    int rc = PPP_OK;
    if (ns > 0) {
        HIPCHK(h, R.sel.ensure((size_t)ns)); HIPCHK(h, R.ord.ensure((size_t)ns));
        HIPCHK(h, hipMemsetAsync(R.ord.p, 0xff, (size_t)ns * sizeof(int), h->stream));
        RegSource S = {source, nullptr, nullptr, nullptr, nullptr, threshold};
        if (source == PPP_REGIONS_UNCOVERED) S.bytes = h->pcov.flags.p;
        else if (source == PPP_REGIONS_OVERLAP) { S.first = h->pcon.first.p; S.last = h->pcon.last.p; }
        else if (source == PPP_REGIONS_NARROW) S.half_width = half_width;
        else {
            HIPCHK(h, R.mask.ensure(N1));
            HIPCHK(h, hipMemcpyAsync(R.mask.p, mask, N, hipMemcpyHostToDevice, h->stream));
            S.bytes = R.mask.p;
        }
        LAUNCH(h, "k_reg_select", k_reg_select, (unsigned)((ns + REG_T - 1) / REG_T), REG_T, 0, h->sorted4.p, ns, S, T, R.sel.p);
        RegSel sel = {R.sel.p, nullptr, R.ord.p, nullptr, nullptr};
        rc = compact(h, sel, ns, R.cnt.p, (int *)R.tot.p + 4, [&](int kept) -> int {
            if (kept < 0 || kept > ns) return fail(h, PPP_ERR_HIP, "regions: selection count corrupt");
            nsel = (size_t)kept;
            HIPCHK(h, R.list.ensure(nsel)); HIPCHK(h, R.parent.ensure(nsel)); HIPCHK(h, R.acc.ensure(nsel));
            sel.list = R.list.p; sel.parent = R.parent.p; sel.acc = R.acc.p;
            return PPP_OK;
        });
        if (rc) return rc;
    }
    if (nsel > 0) {
        const float r2 = link * link;
        int grp = REG_GROUP;
        if (const char *ev = tuning_env("PPP_REG_GROUP")) grp = atoi(ev); /* tuning runs only */
        const unsigned gl = (unsigned)((nsel * (size_t)grp + REG_T - 1) / REG_T), gp = (unsigned)((nsel + REG_T - 1) / REG_T);
#define PPP_REG_LINK(G) LAUNCH(h, "k_reg_link", k_reg_link<G>, gl, REG_T, 0, h->meta.p, h->sorted4.p, h->slab_start.p, h->slab_ytab.p, R.list.p, (int)nsel, R.ord.p, R.parent.p, link, r2, err)
        if (grp == 1) PPP_REG_LINK(1);
        else if (grp == 4) PPP_REG_LINK(4);
        else if (grp == 16) PPP_REG_LINK(16);
        else if (grp == 64) PPP_REG_LINK(64);
        else if (grp == 8) PPP_REG_LINK(8);
        else return fail(h, PPP_ERR_ARG, "regions: PPP_REG_GROUP must be 1, 4, 8, 16 or 64");
#undef PPP_REG_LINK
        LAUNCH(h, "k_reg_flatten", k_reg_flatten, gp, REG_T, 0, h->sorted4.p, R.list.p, (int)nsel, R.parent.p, R.acc.p, T, err);
        LAUNCH(h, "k_reg_labels", k_reg_labels, gp, REG_T, 0, h->sorted4.p, R.list.p, (int)nsel, R.parent.p, R.acc.p, (int)N, R.labels.p,
               R.head_root.p, R.tot.p);
        RegHeadSel heads = {R.labels.p, R.head_root.p, R.acc.p, nullptr};
        rc = compact(h, heads, (int)N, R.cnt.p, (int *)R.tot.p + 5, [&](int kept) -> int {
            if (kept < 0 || (size_t)kept > nsel) return fail(h, PPP_ERR_HIP, "regions: region count corrupt");
            nreg = (size_t)kept;
            HIPCHK(h, R.rows.ensure(nreg));
            heads.rows = R.rows.p;
            return PPP_OK;
        });
        if (rc) return rc;
    }
    HIPCHK(h, copy_sync(h, tot, R.tot.p, 4 * sizeof(unsigned), hipMemcpyDeviceToHost));
    if (tot[3]) return fail(h, PPP_ERR_CAPACITY, "regions: a union-find walk reached its trip cap");
    if (tot[0] != nreg || tot[1] > nreg || tot[2] > nsel) return fail(h, PPP_ERR_HIP, "regions: totals corrupt");
    return PPP_OK;
}

/* the opening of every region call (whole_cloud_begin) and its argument checks */
static int regions_begin(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius)
{
    if (int rcb = whole_cloud_begin(h, "regions", "a region does not stop at a part's border")) return rcb;
    if (source < PPP_REGIONS_UNCOVERED || source > PPP_REGIONS_MASK) return fail(h, PPP_ERR_ARG, "regions: unknown source");
    if (source == PPP_REGIONS_MASK && !mask) return fail(h, PPP_ERR_ARG, "regions: PPP_REGIONS_MASK needs a mask");
    if (source == PPP_REGIONS_NARROW && !(threshold > 0.f && threshold <= 3.402823466e+38f))
        return fail(h, PPP_ERR_ARG, "regions: PPP_REGIONS_NARROW needs a positive finite threshold");
    if (!(fabsf(link_radius) <= 3.402823466e+38f)) return fail(h, PPP_ERR_ARG, "regions: link_radius is not a finite number");
    return PPP_OK;
}

/* could a region's fixed-point sum leave 64 bits?  then no centroid is given (B.34) */
static bool regions_nan_centroid(double reach, size_t selected) { return reach * REG_FIXED * (double)selected >= 4611686018427387904.0; }

int ppp_get_regions(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius, int *labels, size_t cap,
                    ppp_region *regions, size_t region_cap, ppp_region_stats *stats)
{
    { int rca = regions_begin(h, source, mask, threshold, link_radius); if (rca) return rca; }
    if (h->P.slice_begin != 0 || h->P.slice_end != 0)
        return fail(h, PPP_ERR_UNSUPPORTED, "regions: a region does not stop at a range border: a slice-range handle indexes a part of the cloud only");
    const float link = link_radius > 0.f ? link_radius : h->P.normal_radius;
    if (source != PPP_REGIONS_NARROW) threshold = 0.f;
    /* the source's own call: builds its result if the handle does not hold it, answers from it if it does, refuses as it does */
    unsigned long long serial = 0;
    int rc = PPP_OK;
    if (source == PPP_REGIONS_UNCOVERED) { rc = ppp_get_path_coverage(h, nullptr, 0, nullptr, nullptr); serial = h->pcov.serial; }
    else if (source == PPP_REGIONS_OVERLAP) { rc = ppp_get_path_contacts(h, nullptr, nullptr, nullptr, 0, nullptr); serial = h->pcon.serial; }
    else if (source == PPP_REGIONS_NARROW) { rc = ppp_get_contact_field(h, nullptr, nullptr, 0, 0.f, nullptr); serial = h->field.built; }
    if (rc) return rc;
    const size_t N = h->n;
    auto &R = h->regions;
    const bool reuse = source != PPP_REGIONS_MASK && R.valid && R.source == source && R.threshold == threshold && R.link == link &&
                       R.serial == serial && R.stats.n == N;
    if (!reuse) {
        R.valid = false;
        rc = index_ready(h, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
        if (rc) return rc;
        if (h->ranged || h->use_part) return fail(h, PPP_ERR_UNSUPPORTED, "regions: a slice-range handle indexes a part of the cloud only");
        double reach = 0.0; /* the largest |coordinate| of the index */
        for (int d = 0; d < 3; ++d) reach = std::max(reach, std::max(std::fabs((double)h->hmeta.mn[d]), std::fabs((double)h->hmeta.mx[d])));
        size_t nsel = 0, nreg = 0;
        unsigned tot[4];
        rc = regions_compute(h, source, mask, h->field.hw.p, threshold, link, TileRange{-INFINITY, INFINITY, -INFINITY, INFINITY}, nsel, nreg, tot);
        if (rc) return rc;
        ppp_region_stats st = {};
        st.n = N; st.selected = nsel; st.regions = nreg; st.singletons = tot[1]; st.largest = tot[2];
        R.stats = st;
        R.nan_centroid = regions_nan_centroid(reach, nsel);
        R.source = source; R.threshold = threshold; R.link = link; R.serial = serial;
        R.valid = true;
    }
    if (stats) *stats = R.stats;
    const size_t k = std::min(cap, N);
    if (labels && k) HIPCHK(h, copy_sync(h, labels, R.labels.p, k * sizeof(int), hipMemcpyDeviceToHost));
    const size_t kr = std::min(region_cap, R.stats.regions);
    if (regions && kr) {
        std::vector<RegAcc> rows(kr);
        HIPCHK(h, copy_sync(h, rows.data(), R.rows.p, kr * sizeof(RegAcc), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < kr; ++i) {
            const RegAcc &a = rows[i];
            ppp_region &o = regions[i];
            o.label = a.label; o.count = a.count;
            for (int c = 0; c < 3; ++c) {
                o.mn[c] = -ordered_unkey(a.kmn[c]); o.mx[c] = ordered_unkey(a.kmx[c]);
                o.centroid[c] = R.nan_centroid ? (double)NAN : (double)a.sum[c] / (double)a.count / REG_FIXED;
            }
        }
    }
    return PPP_OK;
}

int ppp_get_regions_tile(ppp_handle h, int source, const unsigned char *mask, float threshold, float link_radius, int *labels, size_t cap,
                         ppp_region_part *parts, size_t part_cap, ppp_region_halo *halos, size_t halo_cap, ppp_region_tile_stats *stats)
{
    int rc = regions_begin(h, source, mask, threshold, link_radius);
    if (rc) return rc;
    if (source == PPP_REGIONS_UNCOVERED || source == PPP_REGIONS_OVERLAP)
        return fail(h, PPP_ERR_UNSUPPORTED, "regions tile: a range's coverage knows its own slices' balls only: OR the ranges' flags (ppp_get_path_coverage) and pass the result as a mask (PPP_REGIONS_MASK)");
    const float link = link_radius > 0.f ? link_radius : h->P.normal_radius;
    if (source != PPP_REGIONS_NARROW) threshold = 0.f;
    unsigned long long serial = 0;
    if (source == PPP_REGIONS_NARROW) { /* the field of the owned points and a halo of one link radius */
        rc = ppp_get_contact_field_tile(h, nullptr, nullptr, nullptr, 0, link, 0.f, nullptr);
        if (rc) return rc;
        serial = h->ftile.built;
    }
    const size_t N = h->n;
    auto &Q = h->rtile;
    const bool reuse = source != PPP_REGIONS_MASK && Q.valid && Q.source == source && Q.threshold == threshold && Q.link == link &&
                       Q.serial == serial && Q.stats.n == N;
    if (!reuse) {
        Q.valid = false;
        rc = index_ready(h, false); /* (behind a window pass it keeps that pass's run state, as every API mirror's does) */
        if (rc) return rc;
        TileRange T;
        rc = tile_range(h, link, T);
        if (rc) return rc;
        if (leaves_indexed_range(h, T.ev_lo, T.ev_hi))
            return fail(h, PPP_ERR_CAPACITY, "regions tile: the owned interval widened by the link radius reaches beyond the indexed slice range: raise range_margin");
        const unsigned char *owned_map = h->ftile.owned.p;
        if (source == PPP_REGIONS_MASK) { /* the owned map of this range and link */
            int pos0, pos1;
            rc = tile_positions(h, T, pos0, pos1);
            if (rc) return rc;
            const size_t N1 = std::max<size_t>(N, 1);
            HIPCHK(h, Q.owned.ensure(N1)); HIPCHK(h, Q.cnt.ensure(2));
            HIPCHK(h, hipMemsetAsync(Q.owned.p, 0, N1, h->stream));
            HIPCHK(h, hipMemsetAsync(Q.cnt.p, 0, 2 * sizeof(int), h->stream));
            if (pos1 > pos0)
                LAUNCH(h, "k_tile_mark", k_tile_mark, (unsigned)((pos1 - pos0 + PCON_T - 1) / PCON_T), PCON_T, 0, h->sorted4.p, pos0, pos1, T,
                       Q.owned.p, Q.cnt.p);
            owned_map = Q.owned.p;
        }
        size_t nsel = 0, nreg = 0;
        unsigned tot[4];
        rc = regions_compute(h, source, mask, h->ftile.hw.p, threshold, link, T, nsel, nreg, tot);
        if (rc) return rc;
        /* the tile's view of the device result: labels of the owned points, the components with an owned point, their halo points */
        std::vector<unsigned char> own(N);
        std::vector<RegAcc> rows(nreg);
        Q.labels.assign(N, -1);
        if (N) HIPCHK(h, copy_sync(h, own.data(), owned_map, N, hipMemcpyDeviceToHost));
        if (N && nsel) HIPCHK(h, copy_sync(h, Q.labels.data(), h->regions.labels.p, N * sizeof(int), hipMemcpyDeviceToHost));
        if (nreg) HIPCHK(h, copy_sync(h, rows.data(), h->regions.rows.p, nreg * sizeof(RegAcc), hipMemcpyDeviceToHost));
        Q.parts.clear(); Q.halos.clear();
        size_t selected = 0;
        for (const RegAcc &a : rows) {
            if (!a.count) continue; /* a component of halo points alone: its owners' tiles report it */
            ppp_region_part o;
            o.label = a.label; o.count = a.count;
            for (int c = 0; c < 3; ++c) { o.mn[c] = -ordered_unkey(a.kmn[c]); o.mx[c] = ordered_unkey(a.kmx[c]); o.fsum[c] = a.sum[c]; }
            Q.parts.push_back(o);
            selected += a.count;
        }
        auto has_part = [&](int label) {
            auto it = std::lower_bound(Q.parts.begin(), Q.parts.end(), label, [](const ppp_region_part &r, int l) { return r.label < l; });
            return it != Q.parts.end() && it->label == label;
        };
        for (size_t i = 0; i < N; ++i) {
            if (own[i] == 1 || Q.labels[i] < 0) continue;
            if (own[i] == 2 && has_part(Q.labels[i])) Q.halos.push_back(ppp_region_halo{(int)i, Q.labels[i]});
            Q.labels[i] = -1;
        }
        ppp_region_tile_stats st = {};
        st.n = N; st.selected = selected; st.parts = Q.parts.size(); st.halo_points = Q.halos.size();
        for (int d = 0; d < 3; ++d) /* the whole cloud's bounds: the same on every handle of the cloud */
            st.max_abs_coord = std::max(st.max_abs_coord, std::max(std::fabs((double)h->h_mn[d]), std::fabs((double)h->h_mx[d])));
        st.own_lo = T.own_lo; st.own_hi = T.own_hi;
        Q.stats = st;
        Q.source = source; Q.threshold = threshold; Q.link = link; Q.serial = serial;
        Q.valid = true;
    }
    if (stats) *stats = Q.stats;
    const size_t k = std::min(cap, N), kp = std::min(part_cap, Q.parts.size()), kh = std::min(halo_cap, Q.halos.size());
    if (labels && k) memcpy(labels, Q.labels.data(), k * sizeof(int));
    if (parts && kp) memcpy(parts, Q.parts.data(), kp * sizeof(ppp_region_part));
    if (halos && kh) memcpy(halos, Q.halos.data(), kh * sizeof(ppp_region_halo));
    return PPP_OK;
}

int ppp_merge_region_tiles(size_t tiles, const int *const *labels, const ppp_region_part *const *parts, const ppp_region_halo *const *halos,
                           const ppp_region_tile_stats *stats, int *out_labels, size_t cap, ppp_region *regions, size_t region_cap,
                           ppp_region_stats *out_stats)
{
    if (!tiles || !labels || !parts || !halos || !stats) return PPP_ERR_ARG;
    const size_t N = stats[0].n;
    std::vector<size_t> first(tiles + 1, 0); /* node of (t, part j) = first[t] + j */
    size_t selected = 0;
    double reach = 0.0;
    for (size_t t = 0; t < tiles; ++t) {
        if (stats[t].n != N || !labels[t] || (stats[t].parts && !parts[t]) || (stats[t].halo_points && !halos[t])) return PPP_ERR_ARG;
        for (size_t j = 1; j < stats[t].parts; ++j) if (!(parts[t][j - 1].label < parts[t][j].label)) return PPP_ERR_ARG;
        first[t + 1] = first[t] + stats[t].parts;
        selected += stats[t].selected;
        reach = std::max(reach, stats[t].max_abs_coord);
    }
    auto node_of = [&](size_t t, int label) -> long long { /* -1: tile t has no part of that label */
        const ppp_region_part *b = parts[t], *e = b + stats[t].parts;
        const ppp_region_part *it = std::lower_bound(b, e, label, [](const ppp_region_part &r, int l) { return r.label < l; });
        return it != e && it->label == label ? (long long)(first[t] + (size_t)(it - b)) : -1;
    };
    /* who owns a point: the one tile that labels it */
    std::vector<int> owner(N, -1);
    for (size_t t = 0; t < tiles; ++t)
        for (size_t i = 0; i < N; ++i)
            if (labels[t][i] >= 0) {
                if (owner[i] >= 0) return PPP_ERR_ARG; /* owned twice */
                owner[i] = (int)t;
            }
    const size_t nodes = first[tiles];
    std::vector<size_t> parent(nodes);
    for (size_t v = 0; v < nodes; ++v) parent[v] = v;
    auto find = [&](size_t v) { while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; } return v; };
    for (size_t t = 0; t < tiles; ++t)
        for (size_t e = 0; e < stats[t].halo_points; ++e) {
            const ppp_region_halo &hp = halos[t][e];
            if (hp.cloud_index < 0 || (size_t)hp.cloud_index >= N || owner[(size_t)hp.cloud_index] < 0) return PPP_ERR_ARG; /* nobody's point */
            const size_t u = (size_t)owner[(size_t)hp.cloud_index];
            const long long a = node_of(t, hp.label), b = node_of(u, labels[u][(size_t)hp.cloud_index]);
            if (a < 0 || b < 0) return PPP_ERR_ARG;
            const size_t ra = find((size_t)a), rb = find((size_t)b);
            if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
        }
    /* the merged rows: integer sums, minima and maxima (as ordered keys: the order the device's atomics fold in) */
    struct Row { int label; unsigned long long count; unsigned kmn[3], kmx[3]; long long sum[3]; };
    std::vector<Row> acc(nodes, Row{0x7fffffff, 0, {0, 0, 0}, {0, 0, 0}, {0, 0, 0}});
    for (size_t t = 0; t < tiles; ++t)
        for (size_t j = 0; j < stats[t].parts; ++j) {
            const ppp_region_part &p = parts[t][j];
            Row &r = acc[find(first[t] + j)];
            r.label = std::min(r.label, p.label); r.count += p.count;
            for (int c = 0; c < 3; ++c) {
                r.kmn[c] = std::max(r.kmn[c], ordered_key(-p.mn[c])); r.kmx[c] = std::max(r.kmx[c], ordered_key(p.mx[c]));
                r.sum[c] = (long long)((unsigned long long)r.sum[c] + (unsigned long long)p.fsum[c]);
            }
        }
    std::vector<size_t> roots;
    for (size_t v = 0; v < nodes; ++v) if (parent[v] == v) roots.push_back(v);
    std::sort(roots.begin(), roots.end(), [&](size_t a, size_t b) { return acc[a].label < acc[b].label; });
    ppp_region_stats st = {};
    st.n = N; st.selected = selected; st.regions = roots.size();
    for (size_t v : roots) { st.singletons += acc[v].count == 1; st.largest = std::max(st.largest, (size_t)acc[v].count); }
    if (out_stats) *out_stats = st;
    const bool nan_centroid = regions_nan_centroid(reach, selected);
    const size_t kr = std::min(region_cap, roots.size());
    for (size_t i = 0; regions && i < kr; ++i) {
        const Row &a = acc[roots[i]];
        ppp_region &o = regions[i];
        o.label = a.label; o.count = (unsigned)a.count;
        for (int c = 0; c < 3; ++c) {
            o.mn[c] = -ordered_unkey(a.kmn[c]); o.mx[c] = ordered_unkey(a.kmx[c]);
            o.centroid[c] = nan_centroid ? (double)NAN : (double)a.sum[c] / (double)o.count / REG_FIXED;
        }
    }
    const size_t k = std::min(cap, N);
    for (size_t i = 0; out_labels && i < k; ++i) {
        out_labels[i] = -1;
        if (owner[i] < 0) continue;
        const long long v = node_of((size_t)owner[i], labels[(size_t)owner[i]][i]);
        if (v < 0) return PPP_ERR_ARG; /* a label without its part row */
        out_labels[i] = acc[find((size_t)v)].label;
    }
    return PPP_OK;
}

} // extern "C"
