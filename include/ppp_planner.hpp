/*
 * ppp_planner.hpp -- shared plumbing of the drop-in planner classes (Path_Generate.h,
 * Path_Generate_Algorithm.h, robot_path.h): owns one engine handle, loads the PCD, forwards
 * every method to the C ABI of include/ppp_hip.h.  Header-only on purpose: the reference
 * defines two different classes named path_generater (one per executable), so nothing here
 * may live in a shared translation unit.
 *
 * Types in the public signatures: with Eigen available (-DPPP_WITH_EIGEN or <Eigen/Dense> on
 * the include path) the real Eigen::Vector3f / Vector3d are used; otherwise the three-float
 * stand-ins below, which cover what the reference's callers do with them (construct from
 * three numbers, index with []).  PCL is not needed: the cloud lives in HBM.
 */
#ifndef PPP_PLANNER_HPP
#define PPP_PLANNER_HPP

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ppp_hip.h"

#if defined(PPP_WITH_EIGEN) || (defined(__has_include) && __has_include(<Eigen/Dense>))
#include <Eigen/Dense>
#else
namespace Eigen {
template <typename T>
struct PppVec3 {
    T v[3];
    PppVec3() : v{0, 0, 0} {}
    PppVec3(T a, T b, T c) : v{a, b, c} {}
    T &operator[](int i) { return v[i]; }
    const T &operator[](int i) const { return v[i]; }
    T &operator()(int i) { return v[i]; }
    const T &operator()(int i) const { return v[i]; }
};
typedef PppVec3<float> Vector3f;
typedef PppVec3<double> Vector3d;
} // namespace Eigen
#endif

typedef std::map<double, std::vector<double>> MAP; /* Path_Generate_Algorithm.h:53 */

namespace ppp {

/* Engine handles handed back by the planners of this process, for the next planner to take.  The reference builds a planner
   per workpiece from the file name (path_slicing_alg.cpp:3-30, Path_Generate.cpp:8-33); a handle is a HIP stream plus the
   engine's device buffers and its plan, so the second workpiece of a process pays neither ppp_create nor -- for a cloud of the
   same size and parameters -- the window census (ppp_set_plan_reuse).  A taken handle is given its cloud and parameters
   anew by open(); nothing of the earlier workpiece is readable through it.  PPP_NO_HANDLE_POOL=1 in the environment (or
   HandlePool::keep(0)) switches it off.  Handles still pooled when the process ends go with the HIP runtime. */
class HandlePool {
public:
    static ppp_handle take(int device)
    {
        std::lock_guard<std::mutex> g(mu());
        std::vector<std::pair<int, ppp_handle>> &f = free_list();
        for (size_t i = f.size(); i-- > 0;)
            if (f[i].first == device) {
                ppp_handle h = f[i].second;
                f.erase(f.begin() + (long)i);
                ++reused();
                return h;
            }
        return nullptr;
    }
    static void give(int device, ppp_handle h)
    {
        {
            std::lock_guard<std::mutex> g(mu());
            if (free_list().size() < limit()) {
                free_list().push_back(std::make_pair(device, h));
                return;
            }
        }
        ppp_destroy(h);
    }
    /* how many handles may wait in the pool (default 4; 0 = every planner creates and destroys its own) */
    static void keep(size_t n)
    {
        std::vector<ppp_handle> out;
        {
            std::lock_guard<std::mutex> g(mu());
            limit() = n;
            while (free_list().size() > n) { out.push_back(free_list().back().second); free_list().pop_back(); }
        }
        for (ppp_handle h : out) ppp_destroy(h);
    }
    static size_t taken_from_pool()
    {
        std::lock_guard<std::mutex> g(mu());
        return reused();
    }

private:
    /* (never destroyed: a planner with static storage may hand its handle back after main() has returned) */
    static std::mutex &mu() { static std::mutex *m = new std::mutex; return *m; }
    static std::vector<std::pair<int, ppp_handle>> &free_list() { static auto *f = new std::vector<std::pair<int, ppp_handle>>; return *f; }
    static size_t &reused() { static size_t r = 0; return r; }
    static size_t &limit()
    {
        static size_t n = [] { const char *e = std::getenv("PPP_NO_HANDLE_POOL"); return (e && *e && *e != '0') ? 0 : 4; }();
        return n;
    }
};

/* A resident triangle mesh with its grid (ppp_trimesh): the nominal part as triangles, for the exact deviation.
   Made on a handle's device; it owns its buffers and needs that handle no longer.  Move-only. */
class TriMesh {
public:
    TriMesh() = default;
    ~TriMesh() { ppp_trimesh_destroy(m_); }
    TriMesh(const TriMesh &) = delete;
    TriMesh &operator=(const TriMesh &) = delete;
    TriMesh(TriMesh &&o) noexcept : m_(o.m_), st_(o.st_) { o.m_ = nullptr; }
    TriMesh &operator=(TriMesh &&o) noexcept
    {
        if (this != &o) { ppp_trimesh_destroy(m_); m_ = o.m_; st_ = o.st_; o.m_ = nullptr; }
        return *this;
    }
    /* ppp_default_trimesh_params with what the environment sets: PPP_TRIMESH_CELL (resident units; 0 = automatic) and
       PPP_TRIMESH_ORIENT=viewpoint (every facet normal towards the viewpoint, the origin) */
    static ppp_trimesh_params params_from_env()
    {
        ppp_trimesh_params tp;
        ppp_default_trimesh_params(&tp);
        if (const char *v = std::getenv("PPP_TRIMESH_CELL")) tp.cell = (float)std::atof(v);
        if (const char *v = std::getenv("PPP_TRIMESH_ORIENT")) tp.orient = std::string(v) == "viewpoint" ? PPP_TRIMESH_VIEWPOINT : PPP_TRIMESH_WINDING;
        return tp;
    }
    /* the mesh a caller holds in arrays (tris == nullptr: a soup), or an STL file; tp == nullptr: params_from_env().  The return
       value is ppp_trimesh_create's code; a mesh held before is released first */
    int create(ppp_handle h, const float *verts, size_t n_verts, const int *tris, size_t n_tris, const ppp_trimesh_params *tp = nullptr,
               const float *viewpoint = nullptr)
    {
        const ppp_trimesh_params env = params_from_env();
        ppp_trimesh_destroy(m_);
        m_ = nullptr;
        return ppp_trimesh_create(h, verts, n_verts, tris, n_tris, tp ? tp : &env, viewpoint, &m_, &st_);
    }
    int open_stl(ppp_handle h, const std::string &name, const ppp_trimesh_params *tp = nullptr, const float *viewpoint = nullptr)
    {
        const ppp_trimesh_params env = params_from_env();
        ppp_trimesh_destroy(m_);
        m_ = nullptr;
        return ppp_trimesh_create_stl(h, name.c_str(), tp ? tp : &env, viewpoint, &m_, &st_);
    }
    ppp_trimesh get() const { return m_; }
    explicit operator bool() const { return m_ != nullptr; }
    const ppp_trimesh_stats &stats() const { return st_; }
    /* the welded topology (ppp_trimesh_topology / ppp_trimesh_get_topology), built by the first call: the counts, and
       where asked the maps per triangle and corner of the caller's list -- ids as corner indices 3 f + k, the edge's class, the
       vertex's bits, [3] doubles per corner for each pseudonormal.  The return value is the call's code */
    int topology(ppp_trimesh_topology_stats &st, std::vector<int> *vertex_id = nullptr, std::vector<int> *edge_id = nullptr,
                 std::vector<unsigned char> *edge_class = nullptr, std::vector<unsigned char> *vertex_bits = nullptr,
                 std::vector<double> *vertex_normal = nullptr, std::vector<double> *edge_normal = nullptr) const
    {
        const size_t c = 3 * st_.triangles;
        if (vertex_id) vertex_id->assign(c, -1);
        if (edge_id) edge_id->assign(c, -1);
        if (edge_class) edge_class->assign(c, (unsigned char)255);
        if (vertex_bits) vertex_bits->assign(c, (unsigned char)255);
        if (vertex_normal) vertex_normal->assign(3 * c, 0.0);
        if (edge_normal) edge_normal->assign(3 * c, 0.0);
        return ppp_trimesh_get_topology(m_, vertex_id ? vertex_id->data() : nullptr, edge_id ? edge_id->data() : nullptr,
                                        edge_class ? edge_class->data() : nullptr, vertex_bits ? vertex_bits->data() : nullptr,
                                        vertex_normal ? vertex_normal->data() : nullptr, edge_normal ? edge_normal->data() : nullptr, st_.triangles, &st);
    }

private:
    ppp_trimesh m_ = nullptr;
    ppp_trimesh_stats st_ = {};
};

/* One engine handle + the state every planner class of the reference keeps. */
class Planner {
public:
    Planner() { ppp_default_config(&cfg_); }
    ~Planner()
    {
        if (!h_) return;
        /* every method of the classes returns with its results on the host, so the stream is idle here */
        HandlePool::give(dev_, h_);
    }
    Planner(const Planner &) = delete;
    Planner &operator=(const Planner &) = delete;

    bool ok() const { return h_ != nullptr && loaded_; }
    ppp_handle handle() const { return h_; }
    ppp_config &config() { return cfg_; }

    /* constructor body of the reference classes: load, recolour (no-op here), scale, keep */
    bool open(const std::string &cloud_name)
    {
        if (!acquire()) return false;
        if (is_stl_name(cloud_name)) return open_stl(cloud_name);
        /* pcl::io::loadPCDFile + the x1000 loop: the file's records go straight to HBM (ppp_set_cloud_pcd) */
        size_t n = 0;
        ppp_pcd_layout lay;
        if (ppp_pcd_probe(cloud_name.c_str(), &lay) != PPP_OK) {
            std::fprintf(stderr, "Cloudn't read file!\n"); /* path_slicing_alg.cpp:11 */
            loaded_ = false;
            return false;
        }
        int rc = ppp_set_cloud_pcd(h_, cloud_name.c_str(), &n, nullptr);
        if (rc == PPP_ERR_IO || rc == PPP_ERR_UNSUPPORTED) {
            std::fprintf(stderr, "Cloudn't read file!\n");
            loaded_ = false;
            return false;
        }
        if (rc != PPP_OK) return report(rc);
        loaded_ = true;
        return true;
    }
    /* the handle (from the pool, or a new one) with the configuration's parameters on it */
    bool acquire()
    {
        if (!h_) {
            dev_ = device_from_env();
            h_ = HandlePool::take(dev_);
            if (h_) {
                /* switches a caller may have thrown through handle() on the earlier workpiece: back to the defaults */
                ppp_set_fast_path(h_, 1);
                ppp_enable_timing(h_, 0);
                ppp_set_plan_reuse(h_, 1);
            } else if (ppp_create(dev_, &h_) != PPP_OK) {
                std::fprintf(stderr, "ppp: no MI355X device available (the engine has no CPU fallback)\n");
                h_ = nullptr;
                return false;
            }
        }
        return apply_params();
    }
    /* an STL file as the cloud: its triangles sampled on the device (ppp_set_cloud_stl) with mesh_params_from_env() */
    bool open_stl(const std::string &name)
    {
        const ppp_mesh_params mp = mesh_params_from_env();
        ppp_mesh_stats st;
        const int rc = ppp_set_cloud_stl(h_, name.c_str(), &mp, nullptr, &st);
        if (rc == PPP_ERR_IO) {
            std::fprintf(stderr, "Cloudn't read file!\n");
            loaded_ = false;
            return false;
        }
        if (rc != PPP_OK) { loaded_ = false; return report(rc); }
        std::fprintf(stderr, "ppp: %s: %zu triangles (%zu degenerate, %zu culled) sampled at pitch %g into %zu points\n", name.c_str(), st.triangles,
                     st.degenerate, st.culled, (double)mp.pitch, st.samples);
        loaded_ = true;
        return true;
    }
    /* a name that ends in .stl, in any case: the nominal part as a triangle mesh */
    static bool is_stl_name(const std::string &name)
    {
        const size_t n = name.size();
        return n > 4 && name[n - 4] == '.' && std::tolower((unsigned char)name[n - 3]) == 's' && std::tolower((unsigned char)name[n - 2]) == 't' &&
               std::tolower((unsigned char)name[n - 1]) == 'l';
    }
    /* ppp_default_mesh_params with what the environment sets: PPP_MESH_PITCH (resident units: mm after ChangeRange) and
       PPP_MESH_FACING=front (only the triangles that face the viewpoint, the origin) */
    static ppp_mesh_params mesh_params_from_env()
    {
        ppp_mesh_params mp;
        ppp_default_mesh_params(&mp);
        if (const char *v = std::getenv("PPP_MESH_PITCH")) mp.pitch = (float)std::atof(v);
        if (const char *v = std::getenv("PPP_MESH_FACING")) mp.facing = std::string(v) == "front" ? PPP_MESH_FRONT : PPP_MESH_ALL;
        return mp;
    }
    /* the mesh a caller holds in arrays, sampled into the resident cloud (ppp_set_cloud_mesh; tris == nullptr: a soup).  For a
       planner that was opened before: it replaces that cloud.  mp == nullptr: mesh_params_from_env() */
    bool set_mesh(const float *verts, size_t n_verts, const int *tris, size_t n_tris, const ppp_mesh_params *mp = nullptr,
                  const float *viewpoint = nullptr, ppp_mesh_stats *stats = nullptr)
    {
        if (!acquire()) return false;
        const ppp_mesh_params env = mesh_params_from_env();
        ppp_mesh_stats st;
        const int rc = ppp_set_cloud_mesh(h_, verts, n_verts, tris, n_tris, mp ? mp : &env, viewpoint, nullptr, 0, &st);
        if (stats) *stats = st;
        if (rc != PPP_OK) return report(rc);
        loaded_ = true;
        return true;
    }
    bool remove_outlier(int mean_k, double stddev_mul)
    {
        if (!ok()) return false;
        size_t n = 0;
        int rc = ppp_remove_outlier(h_, mean_k, stddev_mul, &n, nullptr);
        return rc == PPP_OK ? true : report(rc);
    }
    bool voxel_down(float lx, float ly, float lz)
    {
        if (!ok()) return false;
        int overflow = 0;
        int rc = ppp_voxel_down(h_, lx, ly, lz, nullptr, &overflow);
        if (rc == PPP_OK && overflow) std::fprintf(stderr, "[pcl::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. Integer indices would overflow.\n");
        return rc == PPP_OK ? true : report(rc);
    }
    /* SectPath::smooth: MLS on the resident cloud, then the "smooth_<name>" ascii PCD the reference leaves behind
       (path_slicing_alg.cpp:126-138; coordinates back in metres when ChangeRange).  A name with a directory part makes
       an unwritable "smooth_dir/..." path there (pcl::io throws); here the file is skipped with a note. */
    bool smooth_mls(double radius, int order, const std::string &cloud_name, bool scale_back)
    {
        if (!ok()) return false;
        size_t n = 0;
        int rc = ppp_smooth_mls(h_, radius, order, &n);
        if (rc != PPP_OK) return report(rc);
        std::vector<float> xyz(3 * (n ? n : 1));
        rc = ppp_get_cloud(h_, xyz.data(), n, &n);
        if (rc != PPP_OK) return report(rc);
        if (scale_back) for (size_t i = 0; i < 3 * n; ++i) xyz[i] /= 1000;
        const float vp[7] = {0, 0, 0, 1, 0, 0, 0};
        const std::string side = "smooth_" + cloud_name;
        if (ppp_save_pcd(side.c_str(), xyz.data(), n, 3, vp, 0) != PPP_OK) std::fprintf(stderr, "ppp: could not write %s\n", side.c_str());
        return true;
    }
    bool trans2center()
    {
        if (!ok()) return false;
        int rc = ppp_trans2center(h_, nullptr, nullptr, nullptr);
        return rc == PPP_OK ? true : report(rc);
    }
    bool apply_params()
    {
        int rc = ppp_set_params(h_, &cfg_.params);
        return rc == PPP_OK ? true : report(rc);
    }
    bool report(int rc) const
    {
        std::fprintf(stderr, "ppp error %d: %s\n", rc, h_ ? ppp_last_error(h_) : "no handle");
        return false;
    }
    std::vector<int> rangedX_index(int position)
    {
        std::vector<int> out(4096);
        size_t n = 0;
        int rc = ppp_ranged_x_index(h_, position, out.data(), out.size(), &n);
        if (rc == PPP_OK && n > out.size()) { /* the call reports the full count and copies what fits: ask again with room */
            out.resize(n);
            rc = ppp_ranged_x_index(h_, position, out.data(), out.size(), &n);
        }
        if (rc != PPP_OK) { report(rc); n = 0; }
        out.resize(n);
        return out;
    }
    /* estimate_normal() (path_slicing_alg.cpp:141-150, Path_Generation.cpp:323-333): pcl::NormalEstimation, radius 2.5,
       over the whole cloud; the field stays readable as cloud_normals() -- n x (nx ny nz curvature), cloud index order */
    bool estimate_normal()
    {
        if (!ok()) return false;
        size_t n = 0;
        ppp_num_points(h_, &n);
        normals_.assign(4 * n, 0.f);
        int rc = ppp_estimate_normals(h_, normals_.data());
        if (rc != PPP_OK) { normals_.clear(); return report(rc); }
        return true;
    }
    const std::vector<float> &cloud_normals() const { return normals_; }
    size_t num_points() const
    {
        size_t n = 0;
        if (h_) ppp_num_points(h_, &n);
        return n;
    }
    MAP insert_point(const std::vector<int> &indices, float plane_x)
    {
        MAP Node;
        std::vector<double> y(indices.size() + 1), x(indices.size() + 1), z(indices.size() + 1);
        size_t m = 0;
        int rc = ppp_insert_point(h_, indices.data(), indices.size(), plane_x, y.data(), x.data(), z.data(), indices.size(), &m);
        if (rc != PPP_OK) { report(rc); return Node; }
        for (size_t i = 0; i < m; ++i) Node[y[i]] = {x[i], z[i]};
        return Node;
    }
    bool gen_path()
    {
        int rc = ppp_gen_path_async(h_);
        if (rc == PPP_OK) rc = ppp_sync(h_);
        return rc == PPP_OK ? true : report(rc);
    }
    /* coverage of the last pass (ppp_get_coverage: Contact_Path_Generation with the dynamic adjustment only): the cloud's size, the
       covered points and, when asked for, one flag per cloud point */
    bool coverage(size_t &n, size_t &covered, std::vector<unsigned char> *flags = nullptr)
    {
        int rc = ppp_get_coverage(h_, nullptr, 0, &n, &covered);
        if (rc == PPP_OK && flags) {
            flags->assign(n, 0);
            rc = ppp_get_coverage(h_, flags->data(), n, &n, &covered);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* path coverage of the last pass (ppp_get_path_coverage: the contact model on every slice's final path, every walk): the
       cloud's size, the covered points and, when asked for, one flag per cloud point */
    bool path_coverage(size_t &n, size_t &covered, std::vector<unsigned char> *flags = nullptr)
    {
        int rc = ppp_get_path_coverage(h_, nullptr, 0, &n, &covered);
        if (rc == PPP_OK && flags) {
            flags->assign(n, 0);
            rc = ppp_get_path_coverage(h_, flags->data(), n, &n, &covered);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* Path_Generation.cpp:766-770 on path_coverage(): yes / no counted by float ++ (saturating at 2^24 as the reference's do),
       the rate in float (0 / 0 = -nan when there is no pass to measure) */
    void print_path_coverage()
    {
        size_t n = 0, covered = 0;
        if (!path_coverage(n, covered)) n = covered = 0;
        const size_t sat = (size_t)1 << 24;
        float yes = (float)std::min(covered, sat), no = (float)std::min(n - covered, sat), rate;
        rate = yes / (yes + no);
        std::printf("yes: %f, no: %f\n", yes, no);
        std::printf("coverage rate: %f\n", rate);
    }
    /* contact counts of the last pass's paths (ppp_get_path_contacts: how many contact balls of path_coverage() hold each cloud
       point, the first and last slice that has one): the statistics and, when asked for, the three maps by cloud index */
    bool path_contacts(ppp_contact_stats &st, std::vector<unsigned> *counts = nullptr, std::vector<int> *first = nullptr,
                       std::vector<int> *last = nullptr)
    {
        int rc = ppp_get_path_contacts(h_, nullptr, nullptr, nullptr, 0, &st);
        if (rc == PPP_OK && (counts || first || last)) {
            const size_t n = st.n;
            if (counts) counts->assign(n, 0);
            if (first) first->assign(n, -1);
            if (last) last->assign(n, -1);
            rc = ppp_get_path_contacts(h_, counts ? counts->data() : nullptr, first ? first->data() : nullptr,
                                       last ? last->data() : nullptr, n, &st);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* two lines on path_contacts(): the largest and the mean contact count over the covered points, and the points two or more
       slices touch (the overlap bands of neighbouring passes) with their share of the cloud */
    void print_path_contacts()
    {
        ppp_contact_stats st = {};
        if (!path_contacts(st)) st = ppp_contact_stats{};
        const double mean = st.covered ? (double)st.total / (double)st.covered : 0.0;
        const double share = st.n ? (double)st.multi_slice / (double)st.n : 0.0;
        std::printf("contacts: max %u, mean %f over %zu covered points\n", st.max_count, mean, st.covered);
        std::printf("overlap: %zu points touched by two or more slices (%f of the cloud)\n", st.multi_slice, share);
    }
    /* predicted material removal of the last pass's paths (ppp_get_path_removal: the balls of path_contacts(), each weighted by the
       path length its sample stands for and by the profile's pressure at the point, in millimetres of weighted tool travel): the
       statistics and, when asked for, the map by cloud index */
    bool path_removal(ppp_removal_stats &st, int profile = PPP_REMOVAL_HERTZ, std::vector<double> *removal = nullptr)
    {
        int rc = ppp_get_path_removal(h_, profile, nullptr, 0, &st);
        if (rc == PPP_OK && removal) {
            removal->assign(st.n, 0.0);
            rc = ppp_get_path_removal(h_, profile, removal->data(), st.n, &st);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* two lines on path_removal() with the Hertzian profile: the touched points and the length of the path their balls were
       sampled on, then the mean, the smallest and the largest removal over the touched points and cv = the standard deviation /
       the mean, the one figure of how evenly the paths polish */
    void print_path_removal()
    {
        ppp_removal_stats st = {};
        if (!path_removal(st)) st = ppp_removal_stats{};
        const double mean = st.touched ? st.sum / (double)st.touched : 0.0;
        const double var = st.touched ? std::max(0.0, st.sum_sq / (double)st.touched - mean * mean) : 0.0;
        const double cv = mean > 0.0 ? std::sqrt(var) / mean : 0.0;
        std::printf("removal: %zu touched points, path length %f mm\n", st.touched, st.path_length);
        std::printf("removal: mean %f, min %f, max %f, cv %f (mm of Hertz-weighted tool travel)\n", mean, st.touched ? st.min_removal : 0.0,
                    st.touched ? st.max_removal : 0.0, cv);
    }
    /* a dwell schedule for the last pass's paths (ppp_get_path_dwell: a factor per sample of path_contacts()'s table that steers
       path_removal(profile) towards target -- one value per cloud point, or nullptr for "uniform, same total" -- after
       `iterations` rounds, the factors kept in [dwell_min, dwell_max]): the statistics and, when asked for, the rows in (slice,
       sample) order and the map the factors predict.  With a target every call computes again: ask for rows and map at once */
    bool path_dwell(ppp_dwell_stats &st, int profile = PPP_REMOVAL_HERTZ, const std::vector<double> *target = nullptr, int iterations = 8,
                    double dwell_min = 0.25, double dwell_max = 4.0, std::vector<ppp_dwell_row> *rows = nullptr,
                    std::vector<double> *removal = nullptr)
    {
        const double *tg = target ? target->data() : nullptr;
        int rc = ppp_get_path_dwell(h_, profile, tg, iterations, dwell_min, dwell_max, nullptr, 0, nullptr, 0, &st);
        if (rc == PPP_OK && (rows || removal)) {
            if (rows) rows->assign(st.rows, ppp_dwell_row{});
            if (removal) removal->assign(st.n, 0.0);
            rc = ppp_get_path_dwell(h_, profile, tg, iterations, dwell_min, dwell_max, rows ? rows->data() : nullptr, rows ? st.rows : 0,
                                    removal ? removal->data() : nullptr, removal ? st.n : 0, &st);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* two lines on path_dwell() with the Hertzian profile, a uniform target and the default rounds and bounds: the rows, the
       smallest and the largest factor and how many rows ended on a bound, then what the schedule buys -- the rms of (removal -
       target) / level before and after -- and what it costs: the time along the path against the unit feed */
    void print_path_dwell() { print_path_dwell(nullptr); }
    /* the same towards a target map (deviation()'s, one value per cloud point); nullptr: the uniform target */
    void print_path_dwell(const std::vector<double> *target)
    {
        ppp_dwell_stats st = {};
        if (!path_dwell(st, PPP_REMOVAL_HERTZ, target)) st = ppp_dwell_stats{};
        const bool any = st.min_dwell == st.min_dwell;
        std::printf("dwell: %zu samples, factor %f to %f, %zu at the lower and %zu at the upper bound\n", st.rows, any ? st.min_dwell : 1.0,
                    any ? st.max_dwell : 1.0, st.at_min, st.at_max);
        std::printf("dwell: residual %f -> %f after %d rounds, time factor %f\n", st.residual_before == st.residual_before ? st.residual_before : 0.0,
                    st.residual_after == st.residual_after ? st.residual_after : 0.0, st.iterations,
                    st.time_factor == st.time_factor ? st.time_factor : 1.0);
    }
    /* a timed feed schedule for the WayPointsList of the last getPath (ppp_get_path_feed: per waypoint the dwell factor of
       path_dwell() there, the feed of the contact point under fp's cap and acceleration limit, the time at which it is
       reached): the statistics and, when asked for, the rows, one per row of the list.  With a target every call computes
       again: ask for the rows at once */
    bool path_feed(ppp_feed_stats &st, const ppp_feed_params &fp, std::vector<ppp_feed_row> *rows = nullptr, int profile = PPP_REMOVAL_HERTZ,
                   const std::vector<double> *target = nullptr, int iterations = 8, double dwell_min = 0.25, double dwell_max = 4.0)
    {
        const double *tg = target ? target->data() : nullptr;
        size_t W = 0;
        int rc = rows ? ppp_num_waypoints(h_, &W) : PPP_OK;
        if (rc == PPP_OK) {
            if (rows) rows->assign(W, ppp_feed_row{});
            rc = ppp_get_path_feed(h_, profile, tg, iterations, dwell_min, dwell_max, &fp, rows ? rows->data() : nullptr, rows ? W : 0, &st);
        }
        if (rc == PPP_OK && rows && st.W < rows->size()) rows->resize(st.W);
        return rc == PPP_OK ? true : report(rc);
    }
    /* three lines on path_feed() with the default feed parameters, the Hertzian profile, a uniform target and the default
       rounds and bounds: the waypoints by what limits their feed, the feed's range and the lengths, then the duration against
       the nominal one; with feed_file the list's six columns, t and feed go to that file (ppp_write_feed_file); with target
       (deviation()'s map) the dwell schedule steers towards it */
    void print_path_feed(const char *feed_file = nullptr, const std::vector<double> *target = nullptr)
    {
        ppp_feed_params fp;
        ppp_default_feed_params(&fp);
        ppp_feed_stats st = {};
        std::vector<ppp_feed_row> rows;
        if (!path_feed(st, fp, feed_file ? &rows : nullptr, PPP_REMOVAL_HERTZ, target)) { st = ppp_feed_stats{}; rows.clear(); }
        const bool any = st.W > 0;
        std::printf("feed: %zu waypoints on %zu slices: %zu limited by the dwell, %zu by feed_max, %zu by end_feed, %zu by the acceleration\n", st.W,
                    st.slices, st.by_dwell, st.by_feed_max, st.by_end, st.by_accel);
        std::printf("feed: %f to %f mm/s along %f mm of path and %f mm of links\n", any ? st.min_feed : 0.0, any ? st.max_feed : 0.0, st.path_length,
                    st.link_length);
        std::printf("feed: duration %f s (%f s in links), %f s at the nominal feed\n", st.duration, st.duration_links, st.duration_nominal);
        if (!feed_file || !any) return;
        std::vector<float> wp6(6 * st.W);
        size_t W = 0;
        int rc = ppp_get_waypoints(h_, wp6.data(), st.W, &W);
        if (rc != PPP_OK) { report(rc); return; }
        if (W == st.W && ppp_write_feed_file(feed_file, wp6.data(), rows.data(), W) == PPP_OK) std::cout << "File saved: " << feed_file << std::endl;
    }
    /* the deviation map of this planner's cloud, the scan, against the cloud of ref (ppp_get_deviation: per scan point the
       signed distance to the reference surface within dp.max_dist, its mean over dp.smooth_radius, and the target gain *
       max(v - allowance, 0); needs no pass; the two clouds are taken as registered in one frame): the statistics and, when
       asked for, the target by cloud index -- what path_dwell() and path_feed() take as it is -- and the smoothed deviation.
       Every call computes again: ask for the maps at once */
    bool deviation(const Planner &ref, ppp_deviation_stats &st, const ppp_deviation_params &dp, std::vector<double> *target = nullptr,
                   std::vector<double> *smoothed = nullptr, std::vector<unsigned char> *status = nullptr)
    {
        size_t n = 0;
        int rc = (target || smoothed || status) ? ppp_num_points(h_, &n) : PPP_OK;
        if (rc == PPP_OK) {
            if (target) target->assign(n, 0.0);
            if (smoothed) smoothed->assign(n, 0.0);
            if (status) status->assign(n, (unsigned char)PPP_DEV_DROPPED);
            rc = ppp_get_deviation(h_, ref.h_, &dp, nullptr, smoothed ? smoothed->data() : nullptr, nullptr, status ? status->data() : nullptr,
                                   target ? target->data() : nullptr, n, &st);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* deviation() against the triangles themselves (ppp_get_mesh_deviation): per scan point the closest point on the
       nearest triangle of mesh and the offset's component along that facet's own normal -- no pitch, no estimated normal --, then
       deviation()'s smoothing, target and statistics; st.on_face / on_edge / on_vertex say where the closest points lie.  The maps
       asked for come by cloud index */
    bool mesh_deviation(const TriMesh &mesh, ppp_mesh_deviation_stats &st, const ppp_deviation_params &dp, std::vector<double> *target = nullptr,
                        std::vector<double> *smoothed = nullptr, std::vector<unsigned char> *status = nullptr, std::vector<double> *distance = nullptr,
                        std::vector<unsigned char> *region = nullptr)
    {
        size_t n = 0;
        int rc = (target || smoothed || status || distance || region) ? ppp_num_points(h_, &n) : PPP_OK;
        if (rc == PPP_OK) {
            if (target) target->assign(n, 0.0);
            if (smoothed) smoothed->assign(n, 0.0);
            if (status) status->assign(n, (unsigned char)PPP_DEV_DROPPED);
            if (distance) distance->assign(n, 0.0);
            if (region) region->assign(n, (unsigned char)255);
            rc = ppp_get_mesh_deviation(h_, mesh.get(), &dp, nullptr, smoothed ? smoothed->data() : nullptr, distance ? distance->data() : nullptr, nullptr,
                                        region ? region->data() : nullptr, status ? status->data() : nullptr, target ? target->data() : nullptr, n, &st);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* mesh_deviation() with the signed distance in the deviation's place (ppp_get_mesh_signed_deviation): the
       distance to the closest point with the sign of the offset's product with the angle-weighted pseudonormal of the feature it
       lies on -- inside / outside where the mesh is closed (TriMesh::topology()).  feature and flags by cloud index where asked */
    bool mesh_signed_deviation(const TriMesh &mesh, ppp_mesh_signed_deviation_stats &st, const ppp_deviation_params &dp, std::vector<double> *target = nullptr,
                               std::vector<double> *smoothed = nullptr, std::vector<unsigned char> *status = nullptr, std::vector<double> *distance = nullptr,
                               std::vector<unsigned char> *region = nullptr, std::vector<unsigned char> *feature = nullptr,
                               std::vector<unsigned char> *flags = nullptr)
    {
        size_t n = 0;
        int rc = (target || smoothed || status || distance || region || feature || flags) ? ppp_num_points(h_, &n) : PPP_OK;
        if (rc == PPP_OK) {
            if (target) target->assign(n, 0.0);
            if (smoothed) smoothed->assign(n, 0.0);
            if (status) status->assign(n, (unsigned char)PPP_DEV_DROPPED);
            if (distance) distance->assign(n, 0.0);
            if (region) region->assign(n, (unsigned char)255);
            if (feature) feature->assign(n, (unsigned char)255);
            if (flags) flags->assign(n, (unsigned char)0);
            rc = ppp_get_mesh_signed_deviation(h_, mesh.get(), &dp, nullptr, smoothed ? smoothed->data() : nullptr, distance ? distance->data() : nullptr, nullptr,
                                               region ? region->data() : nullptr, feature ? feature->data() : nullptr, flags ? flags->data() : nullptr,
                                               status ? status->data() : nullptr, target ? target->data() : nullptr, n, &st);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* print_deviation()'s three lines for the STL file `name` measured as triangles (TriMesh::params_from_env()), and a fourth:
       the closest points by region and the largest distance.  is_signed: the signed distance (mesh_signed_deviation()), with the
       topology's counts before the block, a warning where the mesh is not closed, and a fifth line: the points by flag and sign */
    void print_mesh_deviation(const std::string &name, const ppp_deviation_params &dp, std::vector<double> *target = nullptr, bool is_signed = false)
    {
        TriMesh mesh;
        ppp_mesh_deviation_stats ms = {};
        const int rc = mesh.open_stl(h_, name);
        if (rc == PPP_ERR_IO) std::fprintf(stderr, "Cloudn't read file!\n");
        else if (rc != PPP_OK) report(rc);
        else
            std::fprintf(stderr, "ppp: %s: %zu triangles (%zu degenerate) in %zu x %zu x %zu cells of %g: %zu pairs, %zu at most in a cell\n", name.c_str(),
                         mesh.stats().triangles, mesh.stats().degenerate, mesh.stats().cells[0], mesh.stats().cells[1], mesh.stats().cells[2],
                         (double)mesh.stats().cell, mesh.stats().pairs, mesh.stats().max_per_cell);
        ppp_mesh_signed_deviation_stats ss = {};
        if (is_signed) {
            ppp_trimesh_topology_stats ts = {};
            const int trc = rc == PPP_OK ? mesh.topology(ts) : rc;
            if (rc == PPP_OK && trc != PPP_OK) std::fprintf(stderr, "ppp: %s: the topology could not be built (code %d)\n", name.c_str(), trc);
            std::printf("topology: %zu vertices, %zu edges: %zu manifold, %zu border, %zu inconsistent, %zu non-manifold; %zu border and %zu irregular vertices\n",
                        ts.vertices, ts.edges, ts.manifold_edges, ts.border_edges, ts.inconsistent_edges, ts.nonmanifold_edges, ts.border_vertices,
                        ts.irregular_vertices);
            if (!ts.closed) std::printf("topology: warning: the mesh is not closed: the sign does not mean inside / outside\n");
            if (rc != PPP_OK || trc != PPP_OK || !mesh_signed_deviation(mesh, ss, dp, target)) { ss = ppp_mesh_signed_deviation_stats{}; if (target) target->clear(); }
            ms = ss.mesh;
        } else if (rc != PPP_OK || !mesh_deviation(mesh, ms, dp, target)) { ms = ppp_mesh_deviation_stats{}; if (target) target->clear(); }
        print_deviation_lines(ms.dev, dp);
        std::printf("deviation: closest points: %zu on a face, %zu on an edge, %zu on a vertex; largest distance %f mm\n", ms.on_face, ms.on_edge,
                    ms.on_vertex, ms.dev.matched ? ms.max_distance : 0.0);
        if (is_signed)
            std::printf("deviation: signed: %zu outside, %zu inside; %zu on the border, %zu on irregular features, %zu by the facet's side\n", ss.positive,
                        ss.negative, ss.on_border, ss.irregular, ss.fallback);
    }
    /* deviation() for the points this planner owns (ppp_get_deviation_tile): this planner holds the scan with a
       slice range (or whole: it then owns everything), ref the reference, whole or a slice range that covers the owned interval
       widened by halo >= dp.max_dist + dp.smooth_radius.  part is what ppp_merge_deviation_tiles takes, with the maps asked for
       here: smoothed, status, target and owned, by cloud index */
    bool deviation_tile(const Planner &ref, ppp_deviation_tile_stats &part, const ppp_deviation_params &dp, float halo,
                        std::vector<double> *target = nullptr, std::vector<double> *smoothed = nullptr,
                        std::vector<unsigned char> *status = nullptr, std::vector<unsigned char> *owned = nullptr)
    {
        size_t n = 0;
        int rc = (target || smoothed || status || owned) ? ppp_num_points(h_, &n) : PPP_OK;
        if (rc == PPP_OK) {
            if (target) target->assign(n, 0.0);
            if (smoothed) smoothed->assign(n, 0.0);
            if (status) status->assign(n, (unsigned char)PPP_DEV_DROPPED);
            if (owned) owned->assign(n, (unsigned char)0);
            rc = ppp_get_deviation_tile(h_, ref.h_, &dp, halo, nullptr, smoothed ? smoothed->data() : nullptr, nullptr,
                                        status ? status->data() : nullptr, target ? target->data() : nullptr, owned ? owned->data() : nullptr, n,
                                        &part);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* the registration terms at T12 (nullptr: the identity) over the points this planner owns (ppp_get_registration_terms_tile;
       DESIGN.md 7o): this planner holds the scan with a slice range (or whole: it then owns everything), ref the reference, whole
       or a slice range that indexes max_dist + its normal_radius around every moved point.  row and part are what
       ppp_merge_registration_terms and ppp_registration_step take */
    bool registration_terms_tile(const Planner &ref, ppp_registration_row &row, ppp_registration_part &part, const ppp_registration_params &rp,
                                 const double *T12 = nullptr)
    {
        const int rc = ppp_get_registration_terms_tile(h_, ref.h_, &rp, T12, &row, &part);
        return rc == PPP_OK ? true : report(rc);
    }
    /* mesh_deviation() for the points this planner owns (ppp_get_mesh_deviation_tile): this planner holds the scan
       with a slice range (or whole: it then owns everything), mesh lives on its device.  The mesh is whole, so there is no halo:
       only this planner's range_margin must cover dp.smooth_radius.  part is what ppp_merge_mesh_deviation_tiles takes, with the
       maps asked for here: smoothed, status, target and owned, by cloud index */
    bool mesh_deviation_tile(const TriMesh &mesh, ppp_mesh_deviation_tile_stats &part, const ppp_deviation_params &dp,
                             std::vector<double> *target = nullptr, std::vector<double> *smoothed = nullptr,
                             std::vector<unsigned char> *status = nullptr, std::vector<unsigned char> *owned = nullptr,
                             std::vector<double> *distance = nullptr, std::vector<unsigned char> *region = nullptr)
    {
        size_t n = 0;
        int rc = (target || smoothed || status || owned || distance || region) ? ppp_num_points(h_, &n) : PPP_OK;
        if (rc == PPP_OK) {
            if (target) target->assign(n, 0.0);
            if (smoothed) smoothed->assign(n, 0.0);
            if (status) status->assign(n, (unsigned char)PPP_DEV_DROPPED);
            if (owned) owned->assign(n, (unsigned char)0);
            if (distance) distance->assign(n, 0.0);
            if (region) region->assign(n, (unsigned char)255);
            rc = ppp_get_mesh_deviation_tile(h_, mesh.get(), &dp, nullptr, smoothed ? smoothed->data() : nullptr, distance ? distance->data() : nullptr,
                                             nullptr, region ? region->data() : nullptr, status ? status->data() : nullptr,
                                             target ? target->data() : nullptr, owned ? owned->data() : nullptr, n, &part);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* the registration terms at T12 (nullptr: the identity) against the triangles of mesh over the points this planner owns
       (ppp_get_mesh_registration_terms_tile).  row and part are what ppp_merge_registration_terms and
       ppp_registration_step take, unchanged; the mesh is whole, so no range condition exists */
    bool mesh_registration_terms_tile(const TriMesh &mesh, ppp_registration_row &row, ppp_registration_part &part, const ppp_registration_params &rp,
                                      const double *T12 = nullptr)
    {
        const int rc = ppp_get_mesh_registration_terms_tile(h_, mesh.get(), &rp, T12, &row, &part);
        return rc == PPP_OK ? true : report(rc);
    }
    /* ppp_default_deviation_params with what the environment sets of PPP_DEVIATION_MAXDIST, PPP_DEVIATION_SMOOTH,
       PPP_DEVIATION_ALLOWANCE and PPP_DEVIATION_GAIN (the example programs' knobs) */
    static ppp_deviation_params deviation_params_env()
    {
        ppp_deviation_params dp;
        ppp_default_deviation_params(&dp);
        if (const char *v = std::getenv("PPP_DEVIATION_MAXDIST")) dp.max_dist = (float)std::atof(v);
        if (const char *v = std::getenv("PPP_DEVIATION_SMOOTH")) dp.smooth_radius = (float)std::atof(v);
        if (const char *v = std::getenv("PPP_DEVIATION_ALLOWANCE")) dp.allowance = std::atof(v);
        if (const char *v = std::getenv("PPP_DEVIATION_GAIN")) dp.gain = std::atof(v);
        return dp;
    }
    /* three lines on deviation(): the scan's points by status, the deviation's range, mean and rms, and the points that stand
       proud of the allowance with the target's sum; the target goes to *target when given */
    void print_deviation(const Planner &ref, const ppp_deviation_params &dp, std::vector<double> *target = nullptr)
    {
        ppp_deviation_stats st = {};
        if (!deviation(ref, st, dp, target)) { st = ppp_deviation_stats{}; if (target) target->clear(); }
        print_deviation_lines(st, dp);
    }
    static void print_deviation_lines(const ppp_deviation_stats &st, const ppp_deviation_params &dp)
    {
        const bool any = st.matched > 0;
        std::printf("deviation: %zu points: %zu matched, %zu too far, %zu without a normal, %zu dropped\n", st.n, st.matched, st.too_far, st.no_normal,
                    st.dropped);
        std::printf("deviation: %f to %f mm, mean %f, rms %f\n", any ? st.min_dev : 0.0, any ? st.max_dev : 0.0, any ? st.mean_dev : 0.0,
                    any ? st.rms_dev : 0.0);
        std::printf("deviation: %zu points proud of %f mm, %zu below the reference, target sum %f\n", st.proud, dp.allowance, st.below, st.target_sum);
    }
    /* point-to-plane ICP of this planner's cloud, the scan, to the cloud of ref (ppp_register): st.T carries a scan
       point into ref's frame -- transform_cloud(st.T) applies it; rows, when asked for, receives the evaluations at T_0 .. T_steps.
       Started at T0 (3 x 4 row-major, nullptr: the identity): ICP needs a start within the basin of the answer.  Needs no pass
       and changes neither cloud */
    bool register_to(const Planner &ref, ppp_registration_stats &st, const ppp_registration_params &rp, const double *T0 = nullptr,
                     std::vector<ppp_registration_row> *rows = nullptr)
    {
        if (rows) rows->assign((size_t)(rp.iterations > 0 ? rp.iterations : 0) + 1, ppp_registration_row{});
        int rc = ppp_register(h_, ref.h_, &rp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0, &st);
        if (rc != PPP_OK) { if (rows) rows->clear(); return report(rc); }
        if (rows) rows->resize(std::min(rows->size(), (size_t)st.steps + 1));
        return true;
    }
    /* the resident cloud moved by T (ppp_transform_cloud; 3 x 4 row-major in double): plan and results are withdrawn, as after
       any change of the cloud; the normals estimate_normal() left are the old cloud's and are dropped */
    bool transform_cloud(const double *T12)
    {
        int rc = ppp_transform_cloud(h_, T12);
        normals_.clear();
        return rc == PPP_OK ? true : report(rc);
    }
    /* ppp_default_registration_params with what the environment sets of PPP_REGISTER_MAXDIST, PPP_REGISTER_ITERATIONS and
       PPP_REGISTER_MINSTEP (the example programs' knobs) */
    static ppp_registration_params registration_params_env()
    {
        ppp_registration_params rp;
        ppp_default_registration_params(&rp);
        if (const char *v = std::getenv("PPP_REGISTER_MAXDIST")) rp.max_dist = (float)std::atof(v);
        if (const char *v = std::getenv("PPP_REGISTER_ITERATIONS")) rp.iterations = std::atoi(v);
        if (const char *v = std::getenv("PPP_REGISTER_MINSTEP")) rp.min_step = std::atof(v);
        return rp;
    }
    /* register_to() from the identity, five lines on it -- the pairs and the rms of the point-to-plane residual before and
       after, the steps with what ended them and the locked unknowns, the three rows of T -- and, with apply, the cloud moved by
       T when the loop converged.  Returns whether the cloud was moved */
    bool print_registration(const Planner &ref, const ppp_registration_params &rp, bool apply = true)
    {
        ppp_registration_stats st = {};
        const bool ran = register_to(ref, st, rp);
        if (!ran) st = ppp_registration_stats{};
        return print_registration_lines(st, rp, ran, apply);
    }
    /* point-to-plane ICP of this planner's cloud, the scan, to the triangles of mesh themselves (ppp_register_mesh):
       register_to() with the exact closest point and the facet's own normal in the place of a sample and its estimated normal --
       no pitch enters the fit, and it is taken on the facets mesh_deviation() measures against.  st, T0 and rows as register_to()'s */
    bool register_mesh(const TriMesh &mesh, ppp_registration_stats &st, const ppp_registration_params &rp, const double *T0 = nullptr,
                       std::vector<ppp_registration_row> *rows = nullptr)
    {
        if (rows) rows->assign((size_t)(rp.iterations > 0 ? rp.iterations : 0) + 1, ppp_registration_row{});
        int rc = ppp_register_mesh(h_, mesh.get(), &rp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0, &st);
        if (rc != PPP_OK) { if (rows) rows->clear(); return report(rc); }
        if (rows) rows->resize(std::min(rows->size(), (size_t)st.steps + 1));
        return true;
    }
    /* print_registration() for the STL file `name` registered to as triangles (TriMesh::params_from_env()): the grid's line on
       stderr, register_mesh() from the identity, print_registration()'s five lines and, with apply, the cloud moved */
    bool print_mesh_registration(const std::string &name, const ppp_registration_params &rp, bool apply = true)
    {
        TriMesh mesh;
        ppp_registration_stats st = {};
        const bool ran = open_mesh_for_registration(mesh, name) && register_mesh(mesh, st, rp);
        if (!ran) st = ppp_registration_stats{};
        return print_registration_lines(st, rp, ran, apply);
    }
    /* the STL file `name` as the triangles a registration runs against: its grid's line on stderr, or why it could not be had */
    bool open_mesh_for_registration(TriMesh &mesh, const std::string &name)
    {
        const int rc = mesh.open_stl(h_, name);
        if (rc == PPP_ERR_IO) std::fprintf(stderr, "Cloudn't read file!\n");
        else if (rc != PPP_OK) report(rc);
        else
            std::fprintf(stderr, "ppp: %s: %zu triangles (%zu degenerate) in %zu x %zu x %zu cells of %g: %zu pairs, %zu at most in a cell\n", name.c_str(),
                         mesh.stats().triangles, mesh.stats().degenerate, mesh.stats().cells[0], mesh.stats().cells[1], mesh.stats().cells[2],
                         (double)mesh.stats().cell, mesh.stats().pairs, mesh.stats().max_per_cell);
        return rc == PPP_OK;
    }
    /* print_registration()'s five lines on the statistics of a chain that ran (or did not), and its move of the cloud */
    bool print_registration_lines(const ppp_registration_stats &st, const ppp_registration_params &rp, bool ran, bool apply)
    {
        std::printf("registration: %zu of %zu points paired, rms %f mm; after %d steps %zu paired, rms %f mm\n", st.pairs_before, st.indexed,
                    st.pairs_before ? st.rms_before : 0.0, st.steps, st.pairs_after, st.pairs_after ? st.rms_after : 0.0);
        std::printf("registration: %s, locked unknowns 0x%02x (rotation x y z, translation x y z from bit 0)\n",
                    st.converged ? "converged" : (ran && st.steps == rp.iterations ? "out of iterations" : "no step possible"), st.locked);
        for (int r = 0; r < 3; ++r) std::printf("registration: T %f %f %f %f\n", st.T[4 * r], st.T[4 * r + 1], st.T[4 * r + 2], st.T[4 * r + 3]);
        return ran && apply && st.converged && transform_cloud(st.T);
    }
    /* trimmed point-to-plane ICP (ppp_register_trimmed): register_to() in which only the share tp.keep of an
       evaluation's pairs with the smallest pair distance enters its sums, for a scan that shows a clamp, a burr or an edge the
       reference does not have.  rows, when asked for, receives the evaluations with their kept / paired counts and cuts;
       status and d2, when asked for, the last evaluation's maps by cloud index (PPP_TRIM_*) */
    bool register_trimmed_to(const Planner &ref, ppp_registration_stats &st, const ppp_trimmed_registration_params &tp, const double *T0 = nullptr,
                             std::vector<ppp_trimmed_registration_row> *rows = nullptr, std::vector<unsigned char> *status = nullptr,
                             std::vector<float> *d2 = nullptr)
    {
        if (rows) rows->assign((size_t)(tp.icp.iterations > 0 ? tp.icp.iterations : 0) + 1, ppp_trimmed_registration_row{});
        size_t n = 0;
        if (status || d2) {
            int rc = ppp_num_points(h_, &n);
            if (rc != PPP_OK) return report(rc);
            if (status) status->assign(n, PPP_TRIM_DROPPED);
            if (d2) d2->assign(n, 0.f);
        }
        int rc = ppp_register_trimmed(h_, ref.h_, &tp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0, status ? status->data() : nullptr,
                                      d2 ? d2->data() : nullptr, n, &st);
        if (rc != PPP_OK) { if (rows) rows->clear(); if (status) status->clear(); if (d2) d2->clear(); return report(rc); }
        if (rows) rows->resize(std::min(rows->size(), (size_t)st.steps + 1));
        return true;
    }
    /* registration_params_env() with keep from PPP_REGISTER_KEEP (the default 0.8 where it is not set) */
    static ppp_trimmed_registration_params trimmed_registration_params_env()
    {
        ppp_trimmed_registration_params tp;
        ppp_default_trimmed_registration_params(&tp);
        tp.icp = registration_params_env();
        if (const char *v = std::getenv("PPP_REGISTER_KEEP")) tp.keep = std::atof(v);
        return tp;
    }
    /* whether PPP_REGISTER_KEEP asks for the trimmed loop: set, and a share below 1 (anything else leaves register_to() as it is) */
    static bool trimmed_registration_asked()
    {
        const char *v = std::getenv("PPP_REGISTER_KEEP");
        return v && v[0] && std::atof(v) < 1.0;
    }
    /* print_registration() on register_trimmed_to(): a line with the kept and the paired counts and the cut before and after,
       then print_registration()'s lines over the kept pairs */
    bool print_registration(const Planner &ref, const ppp_trimmed_registration_params &tp, bool apply = true)
    {
        ppp_registration_stats st = {};
        std::vector<ppp_trimmed_registration_row> rows;
        const bool ran = register_trimmed_to(ref, st, tp, nullptr, &rows);
        if (!ran) st = ppp_registration_stats{};
        const ppp_trimmed_registration_row none = {};
        const ppp_trimmed_registration_row &first = rows.empty() ? none : rows.front(), &last = rows.empty() ? none : rows.back();
        std::printf("registration: keep %f: %zu of %zu pairs kept within %f mm^2; after %d steps %zu of %zu within %f mm^2\n", tp.keep, first.row.pairs,
                    first.paired, first.paired ? first.trim_d2 : 0.0, st.steps, last.row.pairs, last.paired, last.paired ? last.trim_d2 : 0.0);
        std::printf("registration: %zu of %zu points kept, rms %f mm; after %d steps %zu kept, rms %f mm\n", st.pairs_before, st.indexed,
                    st.pairs_before ? st.rms_before : 0.0, st.steps, st.pairs_after, st.pairs_after ? st.rms_after : 0.0);
        std::printf("registration: %s, locked unknowns 0x%02x (rotation x y z, translation x y z from bit 0)\n",
                    st.converged ? "converged" : (ran && st.steps == tp.icp.iterations ? "out of iterations" : "no step possible"), st.locked);
        for (int r = 0; r < 3; ++r) std::printf("registration: T %f %f %f %f\n", st.T[4 * r], st.T[4 * r + 1], st.T[4 * r + 2], st.T[4 * r + 3]);
        return ran && apply && st.converged && transform_cloud(st.T);
    }
    /* robust point-to-plane ICP (ppp_register_robust): register_to() in which every pair is weighed by Tukey's
       biweight of its point-to-plane residual, the scale being 1.4826 times the median absolute residual of each evaluation --
       no share of the scan has to be chosen, as register_trimmed_to()'s keep must be.  rows, when asked for, receives the
       evaluations with their used / paired counts, medians and sigmas; status, weight and residual, when asked for, the last
       evaluation's maps by cloud index (PPP_ROBUST_*) */
    bool register_robust_to(const Planner &ref, ppp_registration_stats &st, const ppp_robust_registration_params &bp, const double *T0 = nullptr,
                            std::vector<ppp_robust_registration_row> *rows = nullptr, std::vector<unsigned char> *status = nullptr,
                            std::vector<float> *weight = nullptr, std::vector<double> *residual = nullptr)
    {
        if (rows) rows->assign((size_t)(bp.icp.iterations > 0 ? bp.icp.iterations : 0) + 1, ppp_robust_registration_row{});
        size_t n = 0;
        if (status || weight || residual) {
            int rc = ppp_num_points(h_, &n);
            if (rc != PPP_OK) return report(rc);
            if (status) status->assign(n, PPP_ROBUST_DROPPED);
            if (weight) weight->assign(n, 0.f);
            if (residual) residual->assign(n, 0.0);
        }
        int rc = ppp_register_robust(h_, ref.h_, &bp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0, status ? status->data() : nullptr,
                                     weight ? weight->data() : nullptr, residual ? residual->data() : nullptr, n, &st);
        if (rc != PPP_OK) {
            if (rows) rows->clear();
            if (status) status->clear();
            if (weight) weight->clear();
            if (residual) residual->clear();
            return report(rc);
        }
        if (rows) rows->resize(std::min(rows->size(), (size_t)st.steps + 1));
        return true;
    }
    /* registration_params_env() with tune from PPP_REGISTER_TUNE and sigma_min from PPP_REGISTER_SIGMA_MIN (the defaults 4.685
       and 1e-4 mm where they are not set) */
    static ppp_robust_registration_params robust_registration_params_env()
    {
        ppp_robust_registration_params bp;
        ppp_default_robust_registration_params(&bp);
        bp.icp = registration_params_env();
        if (const char *v = std::getenv("PPP_REGISTER_TUNE")) bp.tune = std::atof(v);
        if (const char *v = std::getenv("PPP_REGISTER_SIGMA_MIN")) bp.sigma_min = std::atof(v);
        return bp;
    }
    /* print_registration() on register_robust_to(): a line with the used and the paired counts, the median absolute residual
       and sigma before and after, then print_registration()'s lines with the weighted rms */
    bool print_registration(const Planner &ref, const ppp_robust_registration_params &bp, bool apply = true)
    {
        ppp_registration_stats st = {};
        std::vector<ppp_robust_registration_row> rows;
        const bool ran = register_robust_to(ref, st, bp, nullptr, &rows);
        if (!ran) st = ppp_registration_stats{};
        return print_robust_registration_lines(st, bp, rows, ran, apply);
    }
    /* the robust print_registration()'s six lines on the statistics and the rows of a chain that ran (or did not), and its move of
       the cloud */
    bool print_robust_registration_lines(const ppp_registration_stats &st, const ppp_robust_registration_params &bp,
                                         const std::vector<ppp_robust_registration_row> &rows, bool ran, bool apply)
    {
        const ppp_robust_registration_row none = {};
        const ppp_robust_registration_row &first = rows.empty() ? none : rows.front(), &last = rows.empty() ? none : rows.back();
        std::printf("registration: robust, tune %f: %zu of %zu pairs used, median %f mm, sigma %f mm; after %d steps %zu of %zu, median %f mm, sigma %f mm\n",
                    bp.tune, first.used, first.row.pairs, first.row.pairs ? first.median_abs : 0.0, first.row.pairs ? first.sigma : 0.0, st.steps, last.used,
                    last.row.pairs, last.row.pairs ? last.median_abs : 0.0, last.row.pairs ? last.sigma : 0.0);
        std::printf("registration: %zu of %zu points paired, weighted rms %f mm; after %d steps %zu paired, weighted rms %f mm\n", st.pairs_before, st.indexed,
                    first.weight_sum ? st.rms_before : 0.0, st.steps, st.pairs_after, last.weight_sum ? st.rms_after : 0.0);
        std::printf("registration: %s, locked unknowns 0x%02x (rotation x y z, translation x y z from bit 0)\n",
                    st.converged ? "converged" : (ran && st.steps == bp.icp.iterations ? "out of iterations" : "no step possible"), st.locked);
        for (int r = 0; r < 3; ++r) std::printf("registration: T %f %f %f %f\n", st.T[4 * r], st.T[4 * r + 1], st.T[4 * r + 2], st.T[4 * r + 3]);
        return ran && apply && st.converged && transform_cloud(st.T);
    }
    /* robust point-to-plane ICP to the triangles of mesh themselves (ppp_register_mesh_robust): register_mesh()'s
       pairs -- the exact closest point, the facet's own normal -- under register_robust_to()'s weights, for a scan that shows a clamp
       or a strip of the table within max_dist of the part.  st, T0, rows and the maps as register_robust_to()'s; the residual map is
       signed by the facets' winding */
    bool register_mesh_robust(const TriMesh &mesh, ppp_registration_stats &st, const ppp_robust_registration_params &bp, const double *T0 = nullptr,
                              std::vector<ppp_robust_registration_row> *rows = nullptr, std::vector<unsigned char> *status = nullptr,
                              std::vector<float> *weight = nullptr, std::vector<double> *residual = nullptr)
    {
        if (rows) rows->assign((size_t)(bp.icp.iterations > 0 ? bp.icp.iterations : 0) + 1, ppp_robust_registration_row{});
        size_t n = 0;
        if (status || weight || residual) {
            int rc = ppp_num_points(h_, &n);
            if (rc != PPP_OK) return report(rc);
            if (status) status->assign(n, PPP_ROBUST_DROPPED);
            if (weight) weight->assign(n, 0.f);
            if (residual) residual->assign(n, 0.0);
        }
        int rc = ppp_register_mesh_robust(h_, mesh.get(), &bp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0, status ? status->data() : nullptr,
                                          weight ? weight->data() : nullptr, residual ? residual->data() : nullptr, n, &st);
        if (rc != PPP_OK) {
            if (rows) rows->clear();
            if (status) status->clear();
            if (weight) weight->clear();
            if (residual) residual->clear();
            return report(rc);
        }
        if (rows) rows->resize(std::min(rows->size(), (size_t)st.steps + 1));
        return true;
    }
    /* print_mesh_registration() with the robust loop: the grid's line on stderr, register_mesh_robust() from the identity, the
       robust print_registration()'s six lines and, with apply, the cloud moved */
    bool print_mesh_robust_registration(const std::string &name, const ppp_robust_registration_params &bp, bool apply = true)
    {
        TriMesh mesh;
        ppp_registration_stats st = {};
        std::vector<ppp_robust_registration_row> rows;
        const bool ran = open_mesh_for_registration(mesh, name) && register_mesh_robust(mesh, st, bp, nullptr, &rows);
        if (!ran) st = ppp_registration_stats{};
        return print_robust_registration_lines(st, bp, rows, ran, apply);
    }
    /* trimmed point-to-plane ICP to the triangles of mesh themselves (ppp_register_mesh_trimmed): register_mesh()'s
       candidates -- the exact closest point, the facet's own normal -- of which only the share mp.trim.keep with the smallest
       distance enters an evaluation's sums, for a scan more contaminated than register_mesh_robust()'s median bears; with
       mp.border == PPP_MESH_BORDER_REJECT a candidate whose closest point lies on the mesh's border is no pair (the scan's
       overhang beyond an open mesh).  st, T0 and rows as register_trimmed_to()'s, the rows with on_border; status and d2, when
       asked for, the last evaluation's maps by cloud index (PPP_TRIM_*, PPP_MESH_TRIM_BORDER) */
    bool register_mesh_trimmed(const TriMesh &mesh, ppp_registration_stats &st, const ppp_mesh_trimmed_registration_params &mp, const double *T0 = nullptr,
                               std::vector<ppp_mesh_trimmed_registration_row> *rows = nullptr, std::vector<unsigned char> *status = nullptr,
                               std::vector<float> *d2 = nullptr)
    {
        if (rows) rows->assign((size_t)(mp.trim.icp.iterations > 0 ? mp.trim.icp.iterations : 0) + 1, ppp_mesh_trimmed_registration_row{});
        size_t n = 0;
        if (status || d2) {
            int rc = ppp_num_points(h_, &n);
            if (rc != PPP_OK) return report(rc);
            if (status) status->assign(n, PPP_TRIM_DROPPED);
            if (d2) d2->assign(n, 0.f);
        }
        int rc = ppp_register_mesh_trimmed(h_, mesh.get(), &mp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0, status ? status->data() : nullptr,
                                           d2 ? d2->data() : nullptr, n, &st);
        if (rc != PPP_OK) { if (rows) rows->clear(); if (status) status->clear(); if (d2) d2->clear(); return report(rc); }
        if (rows) rows->resize(std::min(rows->size(), (size_t)st.steps + 1));
        return true;
    }
    /* trimmed_registration_params_env() -- keep from PPP_REGISTER_KEEP, 0.8 where it is not set -- with the border rule from
       PPP_REGISTER_BORDER: "reject" is PPP_MESH_BORDER_REJECT, anything else or unset PPP_MESH_BORDER_PAIR */
    static ppp_mesh_trimmed_registration_params mesh_trimmed_registration_params_env()
    {
        ppp_mesh_trimmed_registration_params mp;
        ppp_default_mesh_trimmed_registration_params(&mp);
        mp.trim = trimmed_registration_params_env();
        const char *v = std::getenv("PPP_REGISTER_BORDER");
        mp.border = v && std::string(v) == "reject" ? PPP_MESH_BORDER_REJECT : PPP_MESH_BORDER_PAIR;
        return mp;
    }
    /* print_mesh_registration() with the trimmed loop: the grid's line on stderr, register_mesh_trimmed() from the identity, a line
       with the kept, the paired and the on-border counts and the cut (a distance, mm) before and after, then print_registration()'s
       lines over the kept pairs and, with apply, the cloud moved */
    bool print_mesh_trimmed_registration(const std::string &name, const ppp_mesh_trimmed_registration_params &mp, bool apply = true)
    {
        TriMesh mesh;
        ppp_registration_stats st = {};
        std::vector<ppp_mesh_trimmed_registration_row> rows;
        const bool ran = open_mesh_for_registration(mesh, name) && register_mesh_trimmed(mesh, st, mp, nullptr, &rows);
        if (!ran) st = ppp_registration_stats{};
        const ppp_mesh_trimmed_registration_row none = {};
        const ppp_mesh_trimmed_registration_row &first = rows.empty() ? none : rows.front(), &last = rows.empty() ? none : rows.back();
        std::printf("registration: trimmed to the mesh, keep %f, border %s: %zu of %zu pairs kept, %zu on the border, cut %f mm; after %d steps %zu of %zu, "
                    "%zu on the border, cut %f mm\n", mp.trim.keep, mp.border == PPP_MESH_BORDER_REJECT ? "reject" : "pair", first.trim.row.pairs,
                    first.trim.paired, first.on_border, first.trim.paired ? std::sqrt((double)first.trim.trim_d2) : 0.0, st.steps, last.trim.row.pairs,
                    last.trim.paired, last.on_border, last.trim.paired ? std::sqrt((double)last.trim.trim_d2) : 0.0);
        std::printf("registration: %zu of %zu points kept, rms %f mm; after %d steps %zu kept, rms %f mm\n", st.pairs_before, st.indexed,
                    st.pairs_before ? st.rms_before : 0.0, st.steps, st.pairs_after, st.pairs_after ? st.rms_after : 0.0);
        std::printf("registration: %s, locked unknowns 0x%02x (rotation x y z, translation x y z from bit 0)\n",
                    st.converged ? "converged" : (ran && st.steps == mp.trim.icp.iterations ? "out of iterations" : "no step possible"), st.locked);
        for (int r = 0; r < 3; ++r) std::printf("registration: T %f %f %f %f\n", st.T[4 * r], st.T[4 * r + 1], st.T[4 * r + 2], st.T[4 * r + 3]);
        return ran && apply && st.converged && transform_cloud(st.T);
    }
    /* global registration of this planner's cloud, the scan, to the cloud of ref (ppp_register_global): the starts
       the two clouds' principal frames imply, a coarse chain from each side by side, the fine chain from the cheapest.  st.fine.T
       carries a scan point into ref's frame; cands, when asked for, receives one entry per start.  Needs no pass and no start,
       and changes neither cloud */
    bool register_global_to(const Planner &ref, ppp_global_registration_stats &st, const ppp_global_registration_params &gp,
                            std::vector<ppp_registration_candidate> *cands = nullptr)
    {
        if (cands) cands->assign((size_t)(gp.candidates > 0 ? gp.candidates : 0), ppp_registration_candidate{});
        int rc = ppp_register_global(h_, ref.h_, &gp, cands ? cands->data() : nullptr, cands ? cands->size() : 0, nullptr, 0, &st);
        if (rc != PPP_OK) { if (cands) cands->clear(); return report(rc); }
        return true;
    }
    /* ppp_default_global_registration_params with registration_params_env()'s knobs on the fine chain and, for the coarse stage,
       what the environment sets of PPP_REGISTER_CANDIDATES, PPP_REGISTER_STRIDE and PPP_REGISTER_COARSE_MAXDIST */
    static ppp_global_registration_params global_registration_params_env()
    {
        ppp_global_registration_params gp;
        ppp_default_global_registration_params(&gp);
        gp.fine = registration_params_env();
        if (const char *v = std::getenv("PPP_REGISTER_CANDIDATES")) gp.candidates = std::atoi(v);
        if (const char *v = std::getenv("PPP_REGISTER_STRIDE")) gp.stride = std::atoi(v);
        if (const char *v = std::getenv("PPP_REGISTER_COARSE_MAXDIST")) gp.coarse.max_dist = (float)std::atof(v);
        return gp;
    }
    /* register_global_to(), two lines on the coarse stage -- the queries, the winner with its cost and the second cost: close
       to each other on an ambiguous part -- then print_registration()'s lines on the fine chain and, with apply, the cloud
       moved by T when the fine chain converged.  Returns whether the cloud was moved */
    bool print_global_registration(const Planner &ref, const ppp_global_registration_params &gp, bool apply = true)
    {
        ppp_global_registration_stats g = {};
        const bool ran = register_global_to(ref, g, gp);
        if (!ran) g = ppp_global_registration_stats{};
        return print_global_registration_lines(g, gp, ran, apply);
    }
    /* global registration of this planner's cloud, the scan, to the triangles of mesh themselves (ppp_register_mesh_global;
       DESIGN.md 7x): register_global_to() with the mesh's area frame in the place of a cloud's point frame and register_mesh()'s
       chains in the place of register_to()'s -- no sampled cloud, no pitch, no normal field.  st and cands as register_global_to()'s */
    bool register_mesh_global(const TriMesh &mesh, ppp_global_registration_stats &st, const ppp_global_registration_params &gp,
                              std::vector<ppp_registration_candidate> *cands = nullptr)
    {
        if (cands) cands->assign((size_t)(gp.candidates > 0 ? gp.candidates : 0), ppp_registration_candidate{});
        int rc = ppp_register_mesh_global(h_, mesh.get(), &gp, cands ? cands->data() : nullptr, cands ? cands->size() : 0, nullptr, 0, &st);
        if (rc != PPP_OK) { if (cands) cands->clear(); return report(rc); }
        return true;
    }
    /* print_global_registration() for the STL file `name` registered to as triangles: the grid's line on stderr,
       register_mesh_global(), print_global_registration()'s lines and, with apply, the cloud moved */
    bool print_mesh_global_registration(const std::string &name, const ppp_global_registration_params &gp, bool apply = true)
    {
        TriMesh mesh;
        ppp_global_registration_stats g = {};
        const bool ran = open_mesh_for_registration(mesh, name) && register_mesh_global(mesh, g, gp);
        if (!ran) g = ppp_global_registration_stats{};
        return print_global_registration_lines(g, gp, ran, apply);
    }
    /* print_global_registration()'s seven lines on the statistics of a call that ran (or did not), and its move of the cloud */
    bool print_global_registration_lines(const ppp_global_registration_stats &g, const ppp_global_registration_params &gp, bool ran, bool apply)
    {
        const ppp_registration_stats &st = g.fine;
        std::printf("global registration: %d starts on %zu queries; eigenvalues %f %f %f mm^2 against %f %f %f\n", g.candidates, g.queries,
                    g.scan.eigenvalues[0], g.scan.eigenvalues[1], g.scan.eigenvalues[2], g.ref.eigenvalues[0], g.ref.eigenvalues[1], g.ref.eigenvalues[2]);
        std::printf("global registration: start %d wins at cost %lld, the next other pose at %lld\n", g.winner, g.winner_cost, g.second_cost);
        std::printf("registration: %zu of %zu points paired, rms %f mm; after %d steps %zu paired, rms %f mm\n", st.pairs_before, st.indexed,
                    st.pairs_before ? st.rms_before : 0.0, st.steps, st.pairs_after, st.pairs_after ? st.rms_after : 0.0);
        std::printf("registration: %s, locked unknowns 0x%02x (rotation x y z, translation x y z from bit 0)\n",
                    st.converged ? "converged" : (ran && st.steps == gp.fine.iterations ? "out of iterations" : "no step possible"), st.locked);
        for (int r = 0; r < 3; ++r) std::printf("registration: T %f %f %f %f\n", st.T[4 * r], st.T[4 * r + 1], st.T[4 * r + 2], st.T[4 * r + 3]);
        return ran && apply && st.converged && transform_cloud(st.T);
    }
    const char *path_file() const { return cfg_.path_file; }
    /* the contact field of the resident cloud (ppp_get_contact_field: principal curvatures and the half width r of the contact
       ellipse at every cloud point; needs no pass): the statistics -- narrow counts the points whose contact width 2|r| is below
       min_width -- and, when asked for, the maps by cloud index (curv5: n x 5) */
    bool contact_field(ppp_contact_field_stats &st, std::vector<float> *curv5 = nullptr, std::vector<float> *half_width = nullptr,
                       float min_width = 0.f)
    {
        int rc = ppp_get_contact_field(h_, nullptr, nullptr, 0, min_width, &st);
        if (rc == PPP_OK && (curv5 || half_width)) {
            const size_t n = st.n;
            if (curv5) curv5->assign(5 * n, 0.f);
            if (half_width) half_width->assign(n, 0.f);
            rc = ppp_get_contact_field(h_, curv5 ? curv5->data() : nullptr, half_width ? half_width->data() : nullptr, n, min_width, &st);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* three lines on contact_field(): the points with a contact width, the smallest, mean and largest half width |r|, and the
       points whose contact width 2|r| is below the fixed slice step int(2 * Tool_Radius): equally spaced slices leave a gap there */
    void print_contact_field()
    {
        const int step = (int)(2 * cfg_.params.tool_radius);
        ppp_contact_field_stats st = {};
        if (!contact_field(st, nullptr, nullptr, (float)step)) st = ppp_contact_field_stats{};
        const double mean = st.valid ? st.sum_abs_r / (double)st.valid : 0.0;
        std::printf("contact field: %zu of %zu points have a contact width\n", st.valid, st.n);
        std::printf("half width |r|: min %f, mean %f, max %f\n", st.valid ? st.min_abs_r : 0.f, mean, st.valid ? st.max_abs_r : 0.f);
        std::printf("narrow: %zu points with a contact width below the slice step %d\n", st.narrow, step);
    }
    /* connected regions of the points a contact query singles out (ppp_get_regions: by default the points path_coverage() does
       not flag, linked within link_radius, <= 0: normal_radius): the statistics and, when asked for, the region rows in ascending
       label and the label of every cloud point (-1: not selected) */
    bool regions(ppp_region_stats &st, std::vector<ppp_region> *rows = nullptr, std::vector<int> *labels = nullptr,
                 int source = PPP_REGIONS_UNCOVERED, const unsigned char *mask = nullptr, float threshold = 0.f, float link_radius = 0.f)
    {
        int rc = ppp_get_regions(h_, source, mask, threshold, link_radius, nullptr, 0, nullptr, 0, &st);
        if (rc == PPP_OK && (rows || labels)) {
            if (rows) rows->assign(st.regions, ppp_region{});
            if (labels) labels->assign(st.n, -1);
            rc = ppp_get_regions(h_, source, mask, threshold, link_radius, labels ? labels->data() : nullptr, labels ? st.n : 0,
                                 rows ? rows->data() : nullptr, rows ? st.regions : 0, &st);
        }
        return rc == PPP_OK ? true : report(rc);
    }
    /* where the planned paths leave the workpiece untouched: the uncovered points as regions -- one line of totals, one line per
       region of at least PPP_GAPS_MIN points (environment, default 10), largest first and ties by label, and the count of the
       smaller ones */
    void print_gaps()
    {
        const char *ev = std::getenv("PPP_GAPS_MIN");
        const long least = ev && std::atol(ev) > 0 ? std::atol(ev) : 10;
        ppp_region_stats st = {};
        std::vector<ppp_region> rows;
        if (!regions(st, &rows)) { st = ppp_region_stats{}; rows.clear(); }
        std::printf("gaps: %zu of %zu points uncovered in %zu regions (link %g mm)\n", st.selected, st.n, st.regions,
                    (double)cfg_.params.normal_radius);
        std::vector<const ppp_region *> big;
        for (const ppp_region &r : rows)
            if ((long)r.count >= least) big.push_back(&r);
        std::stable_sort(big.begin(), big.end(), [](const ppp_region *a, const ppp_region *b) { return a->count > b->count; });
        for (const ppp_region *r : big)
            std::printf("gap %d: %u points, x [%f, %f] y [%f, %f], centre (%f, %f, %f)\n", r->label, r->count, r->mn[0], r->mx[0], r->mn[1],
                        r->mx[1], r->centroid[0], r->centroid[1], r->centroid[2]);
        std::printf("gaps: %zu regions below %ld points\n", rows.size() - big.size(), least);
    }
    /* getPath(): returns the list and writes pathFile exactly like path_translation_alg.cpp:216-228 */
    bool get_path(std::vector<float> &wp6)
    {
        int rc = ppp_get_path_async(h_);
        if (rc == PPP_OK) rc = ppp_sync(h_);
        if (rc != PPP_OK) return report(rc);
        size_t W = 0;
        ppp_num_waypoints(h_, &W);
        wp6.resize(6 * W);
        rc = ppp_get_waypoints(h_, wp6.data(), W, &W);
        if (rc != PPP_OK) return report(rc);
        std::cout << "!!!!! GOT PATH !!!!!" << std::endl;
        if (ppp_write_path_file(cfg_.path_file, wp6.data(), W) == PPP_OK) std::cout << "File saved: " << cfg_.path_file << std::endl;
        return true;
    }
    int num_slices()
    {
        int S = 0;
        ppp_num_slices(h_, &S);
        return S;
    }
    /* show() (path_slicing_alg.cpp:69-80, Path_Generation.cpp:37-51) opens a PCLVisualizer on `other_cloud + cloud`: the
       spline knots insert_point added (coloured node_rgb: red, white in contour_alg.cpp:228-230) followed by the cloud itself,
       white, with the cloud point nearest to every millimetre of every path recoloured path_rgb (drawpath,
       path_slicing_alg.cpp:269-288).  No viewer here: with PPP_SHOW_PCD=<file> in the environment that very cloud is written
       as a PointXYZRGB PCD (binary) for any viewer; without it a notice is printed.  with_boundaries: the planner with the
       dynamic adjustment also paints, before it adjusts a slice, the boundary curve it adjusts it against
       (drawpath(*boundary, 0,255,0), path_dynamic_alg.cpp:320-322); slices are painted in the order thread_worker takes them
       (the start slice, then step by step outwards; the reference's two threads interleave as they please -- here left before
       right), so a later curve recolours an earlier one where they share a cloud point, as there. */
    void show_dump(const unsigned char node_rgb[3], const unsigned char path_rgb[3], bool with_boundaries = false)
    {
        const char *out = std::getenv("PPP_SHOW_PCD");
        if (!out || !out[0] || !ok()) {
            std::printf("show(): viewer not built; the cloud stays resident on the GPU (PPP_SHOW_PCD=<file> writes what the viewer would show)\n");
            return;
        }
        size_t n = 0;
        if (ppp_get_cloud(h_, nullptr, 0, &n) != PPP_OK) { report(PPP_ERR_ARG); return; }
        std::vector<float> cloud(3 * (n ? n : 1));
        if (n && ppp_get_cloud(h_, cloud.data(), n, &n) != PPP_OK) { report(PPP_ERR_HIP); return; }
        std::vector<unsigned char> crgb(3 * (n ? n : 1), 255);
        std::vector<float> nodes;
        int S = 0;
        if (ppp_num_slices(h_, &S) != PPP_OK) S = 0; /* show() before GenPath: the bare cloud */
        /* drawpath: dy = miny; while (dy < maxy) { nearest cloud point of path.point(dy) takes the colour; dy += 1; } */
        auto samples = [](double miny, double maxy) {
            std::vector<double> q;
            for (double dy = miny; dy < maxy; dy += 1) q.push_back(dy);
            return q;
        };
        auto paint = [&](const std::vector<double> &xyz, const unsigned char rgb[3]) {
            std::vector<float> qf(xyz.begin(), xyz.end());
            std::vector<int> nn(qf.size() / 3, -1);
            if (nn.empty() || ppp_nearest(h_, qf.data(), nn.size(), nn.data()) != PPP_OK) return;
            for (int id : nn) if (id >= 0 && (size_t)id < n) for (int c = 0; c < 3; ++c) crgb[3 * (size_t)id + c] = rgb[c];
        };
        /* painting order: by the slice's step in its chain when the boundaries are painted too, else as the slices stand */
        std::vector<std::pair<int, int>> order;
        for (int s = 0; s < S; ++s) {
            int step = s;
            if (with_boundaries && ppp_get_boundary(h_, s, nullptr, nullptr, nullptr, 0, nullptr, &step) != PPP_OK) step = s;
            order.push_back(std::make_pair(step, s));
        }
        if (with_boundaries) std::sort(order.begin(), order.end());
        std::vector<std::vector<float>> slice_nodes(S > 0 ? S : 0);
        const unsigned char green[3] = {0, 255, 0};
        size_t painted_boundaries = 0;
        for (const auto &os : order) {
            const int s = os.second;
            if (with_boundaries) {
                size_t mb = 0;
                if (ppp_get_boundary(h_, s, nullptr, nullptr, nullptr, 0, &mb, nullptr) == PPP_OK && mb >= 3) {
                    std::vector<double> by(mb), bx(mb), bz(mb);
                    ppp_spline sp = nullptr;
                    if (ppp_get_boundary(h_, s, by.data(), bx.data(), bz.data(), mb, &mb, nullptr) == PPP_OK &&
                        ppp_spline_create(device_from_env(), mb, by.data(), bx.data(), bz.data(), &sp) == PPP_OK) {
                        const std::vector<double> q = samples(by.front(), by.back());
                        std::vector<double> xyz(3 * q.size());
                        if (!q.empty() && ppp_spline_eval(sp, q.data(), q.size(), xyz.data()) == PPP_OK) { paint(xyz, green); ++painted_boundaries; }
                        ppp_spline_destroy(sp);
                    }
                }
            }
            size_t m = 0;
            if (ppp_get_nodes(h_, s, nullptr, nullptr, nullptr, 0, &m) != PPP_OK || m < 3) continue;
            std::vector<double> y(m), x(m), z(m);
            ppp_get_nodes(h_, s, y.data(), x.data(), z.data(), m, &m);
            for (size_t i = 0; i < m; ++i) { slice_nodes[s].push_back((float)x[i]); slice_nodes[s].push_back((float)y[i]); slice_nodes[s].push_back((float)z[i]); }
            const std::vector<double> q = samples(y.front(), y.back());
            if (q.empty()) continue;
            std::vector<double> xyz(3 * q.size());
            if (ppp_eval_spline(h_, s, q.data(), q.size(), xyz.data()) != PPP_OK) continue;
            paint(xyz, path_rgb);
        }
        if (on_env("PPP_SHOW_WIDTH")) { /* the workpiece as the contact model sees it: every point by |r| / Tool_Radius, no width yellow */
            ppp_contact_field_stats fs = {};
            std::vector<float> hw(n ? n : 1);
            /* (asked of the handle itself: where the call is refused -- a slice-range or part handle -- the dump goes on without) */
            if (ppp_get_contact_field(h_, nullptr, hw.data(), n, 0.f, &fs) == PPP_OK && fs.n == n) {
                for (size_t i = 0; i < n; ++i) {
                    const double a = std::fabs((double)hw[i]);
                    if (a <= 3.402823466e+38) ramp_rgb(a / cfg_.params.tool_radius, &crgb[3 * i]);
                    else { crgb[3 * i] = 255; crgb[3 * i + 1] = 255; crgb[3 * i + 2] = 0; }
                }
                std::printf("show(): %zu points painted by contact half width over Tool_Radius, %zu have none\n", fs.valid, n - fs.valid);
            }
        }
        const bool show_contacts = S > 0 && on_env("PPP_SHOW_CONTACTS");
        if (show_contacts) { /* the dwell of the plan: every point by its contact count on a fixed ramp, the uncovered yellow */
            if (on_env("PPP_SHOW_COVERAGE")) std::printf("show(): PPP_SHOW_CONTACTS paints over PPP_SHOW_COVERAGE\n");
            ppp_contact_stats st = {};
            std::vector<unsigned> cnt;
            if (path_contacts(st, &cnt) && st.n == n) {
                for (size_t i = 0; i < n; ++i) contact_rgb(cnt[i], st.max_count, &crgb[3 * i]);
                std::printf("show(): %zu points painted by contact count (max %u), %zu left uncovered\n", st.covered, st.max_count,
                            n - st.covered);
            }
        }
        if (S > 0 && !show_contacts && on_env("PPP_SHOW_COVERAGE")) { /* the gaps of the plan: every point path coverage leaves uncovered, in yellow */
            std::vector<unsigned char> cov;
            size_t nc = 0, covered = 0;
            if (path_coverage(nc, covered, &cov) && nc == n) {
                for (size_t i = 0; i < n; ++i)
                    if (!cov[i]) { crgb[3 * i] = 255; crgb[3 * i + 1] = 255; crgb[3 * i + 2] = 0; }
                std::printf("show(): %zu points left uncovered by the paths painted\n", n - covered);
            }
        }
        for (int s = 0; s < S; ++s) nodes.insert(nodes.end(), slice_nodes[s].begin(), slice_nodes[s].end()); /* other_cloud: in slice order */
        if (with_boundaries) std::printf("show(): %zu boundary curves painted\n", painted_boundaries);
        const size_t nn_ = nodes.size() / 3;
        std::vector<float> all(nodes);
        all.insert(all.end(), cloud.begin(), cloud.begin() + 3 * n);
        std::vector<unsigned char> rgb(3 * nn_);
        for (size_t i = 0; i < nn_; ++i) for (int c = 0; c < 3; ++c) rgb[3 * i + c] = node_rgb[c];
        rgb.insert(rgb.end(), crgb.begin(), crgb.begin() + 3 * n);
        const float vp[7] = {0, 0, 0, 1, 0, 0, 0};
        if (ppp_save_pcd_rgb(out, all.data(), rgb.data(), nn_ + n, vp, 1) == PPP_OK)
            std::printf("show(): %zu inserted nodes + %zu cloud points written to %s\n", nn_, n, out);
        else std::fprintf(stderr, "ppp: could not write %s\n", out);
    }
    /* PPP_SHOW_CONTACTS's ramp on t = count / max_count: blue (t -> 0) through cyan (1/3) and green (2/3) to red (1); a count of
       0 is yellow, as PPP_SHOW_COVERAGE paints the uncovered points */
    static void contact_rgb(unsigned count, unsigned max_count, unsigned char rgb[3])
    {
        if (!count || !max_count) { rgb[0] = 255; rgb[1] = 255; rgb[2] = 0; return; }
        ramp_rgb((double)count / (double)max_count, rgb);
    }
    /* the ramp itself, t clamped to [0, 1] (PPP_SHOW_WIDTH paints |r| / Tool_Radius with it; both paint over the paths) */
    static void ramp_rgb(double t_in, unsigned char rgb[3])
    {
        const double t = std::min(1.0, std::max(0.0, t_in));
        double r, g, b;
        if (t < 1.0 / 3) { r = 0; g = 3 * t; b = 1; }
        else if (t < 2.0 / 3) { r = 0; g = 1; b = 1 - 3 * (t - 1.0 / 3); }
        else { r = 3 * (t - 2.0 / 3); g = 1 - 3 * (t - 2.0 / 3); b = 0; }
        rgb[0] = (unsigned char)std::lround(255 * r); rgb[1] = (unsigned char)std::lround(255 * g); rgb[2] = (unsigned char)std::lround(255 * b);
    }
    void show_notice()
    {   /* the classes without a colour scheme of their own */
        const unsigned char red[3] = {255, 0, 0};
        show_dump(red, red);
    }
    static bool on_env(const char *name)
    {
        const char *v = std::getenv(name);
        return v && v[0] == '1';
    }
    static int device_from_env()
    {
        const char *e = std::getenv("PPP_DEVICE");
        return e ? std::atoi(e) : 0;
    }

private:
    ppp_handle h_ = nullptr;
    int dev_ = 0;
    ppp_config cfg_;
    bool loaded_ = false;
    std::vector<float> normals_;
};

/* register_to() for a scan held as slice-range planners (ppp_register_tiles): tiles[i] holds the scan with range
   i, refs[i] its reference (one whole-cloud planner may stand in every slot).  st.reg is register_to()'s st, bit for bit, for
   ranges that tile the walk; every evaluation is a host round trip.  A tile's error is reported with its index */
inline bool register_tiles(std::vector<Planner *> &tiles, std::vector<Planner *> &refs, ppp_register_tiles_stats &st,
                           const ppp_registration_params &rp, const double *T0 = nullptr, std::vector<ppp_registration_row> *rows = nullptr)
{
    if (tiles.empty() || refs.size() != tiles.size()) { std::fprintf(stderr, "ppp error %d: register_tiles: one reference per tile\n", PPP_ERR_ARG); return false; }
    std::vector<ppp_handle> hs, rs;
    for (size_t i = 0; i < tiles.size(); ++i) { hs.push_back(tiles[i] ? tiles[i]->handle() : nullptr); rs.push_back(refs[i] ? refs[i]->handle() : nullptr); }
    if (rows) rows->assign((size_t)(rp.iterations > 0 ? rp.iterations : 0) + 1, ppp_registration_row{});
    const int rc = ppp_register_tiles(hs.data(), rs.data(), hs.size(), &rp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0, &st);
    if (rc != PPP_OK) {
        if (rows) rows->clear();
        const ppp_handle at = hs[st.failed_tile >= 0 ? (size_t)st.failed_tile : 0];
        std::fprintf(stderr, "ppp error %d: tile %d: %s\n", rc, st.failed_tile, at ? ppp_last_error(at) : "no handle");
        return false;
    }
    if (rows) rows->resize(std::min(rows->size(), (size_t)st.reg.steps + 1));
    return true;
}

/* register_trimmed_to() for a scan held as slice-range planners (ppp_register_trimmed_tiles): tiles and refs as
   register_tiles() takes them.  st.reg and rows are register_trimmed_to()'s, bit for bit, for ranges that tile the walk; an
   evaluation is four host round trips.  status, d2 and owned, when asked for, receive one map per tile by cloud index: an
   indexed point the tile owns has owned 1 and its PPP_TRIM_* status and d2, every other entry owned 0, PPP_TRIM_DROPPED and NaN */
inline bool register_trimmed_tiles(std::vector<Planner *> &tiles, std::vector<Planner *> &refs, ppp_register_tiles_stats &st,
                                   const ppp_trimmed_registration_params &tp, const double *T0 = nullptr,
                                   std::vector<ppp_trimmed_registration_row> *rows = nullptr, std::vector<std::vector<unsigned char>> *status = nullptr,
                                   std::vector<std::vector<float>> *d2 = nullptr, std::vector<std::vector<unsigned char>> *owned = nullptr)
{
    if (tiles.empty() || refs.size() != tiles.size()) { std::fprintf(stderr, "ppp error %d: register_trimmed_tiles: one reference per tile\n", PPP_ERR_ARG); return false; }
    std::vector<ppp_handle> hs, rs;
    for (size_t i = 0; i < tiles.size(); ++i) { hs.push_back(tiles[i] ? tiles[i]->handle() : nullptr); rs.push_back(refs[i] ? refs[i]->handle() : nullptr); }
    if (rows) rows->assign((size_t)(tp.icp.iterations > 0 ? tp.icp.iterations : 0) + 1, ppp_trimmed_registration_row{});
    size_t n = 0;
    if ((status || d2 || owned) && hs[0]) {
        const int rc = ppp_num_points(hs[0], &n);
        if (rc != PPP_OK) { std::fprintf(stderr, "ppp error %d: tile 0: %s\n", rc, ppp_last_error(hs[0])); return false; }
    }
    std::vector<unsigned char *> sp, op;
    std::vector<float *> dp;
    if (status) { status->assign(hs.size(), std::vector<unsigned char>(n, PPP_TRIM_DROPPED)); for (auto &m : *status) sp.push_back(m.data()); }
    if (d2) { d2->assign(hs.size(), std::vector<float>(n, 0.f)); for (auto &m : *d2) dp.push_back(m.data()); }
    if (owned) { owned->assign(hs.size(), std::vector<unsigned char>(n, 0)); for (auto &m : *owned) op.push_back(m.data()); }
    const int rc = ppp_register_trimmed_tiles(hs.data(), rs.data(), hs.size(), &tp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0,
                                              status ? sp.data() : nullptr, d2 ? dp.data() : nullptr, owned ? op.data() : nullptr, n, &st);
    if (rc != PPP_OK) {
        if (rows) rows->clear();
        if (status) status->clear();
        if (d2) d2->clear();
        if (owned) owned->clear();
        const ppp_handle at = hs[st.failed_tile >= 0 ? (size_t)st.failed_tile : 0];
        std::fprintf(stderr, "ppp error %d: tile %d: %s\n", rc, st.failed_tile, at ? ppp_last_error(at) : "no handle");
        return false;
    }
    if (rows) rows->resize(std::min(rows->size(), (size_t)st.reg.steps + 1));
    return true;
}

/* register_robust_to() for a scan held as slice-range planners (ppp_register_robust_tiles): tiles and refs as
   register_tiles() takes them.  st.reg and rows are register_robust_to()'s, bit for bit, for ranges that tile the walk -- the
   median is the merged histograms', never a tile's own --; an evaluation is four host round trips.  status, weight, residual
   and owned, when asked for, receive one map per tile by cloud index: an indexed point the tile owns has owned 1 and its
   PPP_ROBUST_* status, weight and residual, every other entry owned 0, PPP_ROBUST_DROPPED and NaN */
inline bool register_robust_tiles(std::vector<Planner *> &tiles, std::vector<Planner *> &refs, ppp_register_tiles_stats &st,
                                  const ppp_robust_registration_params &bp, const double *T0 = nullptr,
                                  std::vector<ppp_robust_registration_row> *rows = nullptr, std::vector<std::vector<unsigned char>> *status = nullptr,
                                  std::vector<std::vector<float>> *weight = nullptr, std::vector<std::vector<double>> *residual = nullptr,
                                  std::vector<std::vector<unsigned char>> *owned = nullptr)
{
    if (tiles.empty() || refs.size() != tiles.size()) { std::fprintf(stderr, "ppp error %d: register_robust_tiles: one reference per tile\n", PPP_ERR_ARG); return false; }
    std::vector<ppp_handle> hs, rs;
    for (size_t i = 0; i < tiles.size(); ++i) { hs.push_back(tiles[i] ? tiles[i]->handle() : nullptr); rs.push_back(refs[i] ? refs[i]->handle() : nullptr); }
    if (rows) rows->assign((size_t)(bp.icp.iterations > 0 ? bp.icp.iterations : 0) + 1, ppp_robust_registration_row{});
    size_t n = 0;
    if ((status || weight || residual || owned) && hs[0]) {
        const int rc = ppp_num_points(hs[0], &n);
        if (rc != PPP_OK) { std::fprintf(stderr, "ppp error %d: tile 0: %s\n", rc, ppp_last_error(hs[0])); return false; }
    }
    std::vector<unsigned char *> sp, op;
    std::vector<float *> wp;
    std::vector<double *> rp;
    if (status) { status->assign(hs.size(), std::vector<unsigned char>(n, PPP_ROBUST_DROPPED)); for (auto &m : *status) sp.push_back(m.data()); }
    if (weight) { weight->assign(hs.size(), std::vector<float>(n, 0.f)); for (auto &m : *weight) wp.push_back(m.data()); }
    if (residual) { residual->assign(hs.size(), std::vector<double>(n, 0.0)); for (auto &m : *residual) rp.push_back(m.data()); }
    if (owned) { owned->assign(hs.size(), std::vector<unsigned char>(n, 0)); for (auto &m : *owned) op.push_back(m.data()); }
    const int rc = ppp_register_robust_tiles(hs.data(), rs.data(), hs.size(), &bp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0,
                                             status ? sp.data() : nullptr, weight ? wp.data() : nullptr, residual ? rp.data() : nullptr,
                                             owned ? op.data() : nullptr, n, &st);
    if (rc != PPP_OK) {
        if (rows) rows->clear();
        if (status) status->clear();
        if (weight) weight->clear();
        if (residual) residual->clear();
        if (owned) owned->clear();
        const ppp_handle at = hs[st.failed_tile >= 0 ? (size_t)st.failed_tile : 0];
        std::fprintf(stderr, "ppp error %d: tile %d: %s\n", rc, st.failed_tile, at ? ppp_last_error(at) : "no handle");
        return false;
    }
    if (rows) rows->resize(std::min(rows->size(), (size_t)st.reg.steps + 1));
    return true;
}

/* register_mesh() for a scan held as slice-range planners (ppp_register_mesh_tiles): tiles[i] holds the scan with
   range i, meshes[i] is the mesh on its device (one TriMesh may stand in every slot when all tiles share a device).  st.reg is
   register_mesh()'s st, bit for bit, for ranges that tile the walk; every evaluation is a host round trip.  A tile's error is
   reported with its index */
inline bool register_mesh_tiles(std::vector<Planner *> &tiles, std::vector<TriMesh *> &meshes, ppp_register_tiles_stats &st,
                                const ppp_registration_params &rp, const double *T0 = nullptr, std::vector<ppp_registration_row> *rows = nullptr)
{
    if (tiles.empty() || meshes.size() != tiles.size()) { std::fprintf(stderr, "ppp error %d: register_mesh_tiles: one mesh per tile\n", PPP_ERR_ARG); return false; }
    std::vector<ppp_handle> hs;
    std::vector<ppp_trimesh> ms;
    for (size_t i = 0; i < tiles.size(); ++i) { hs.push_back(tiles[i] ? tiles[i]->handle() : nullptr); ms.push_back(meshes[i] ? meshes[i]->get() : nullptr); }
    if (rows) rows->assign((size_t)(rp.iterations > 0 ? rp.iterations : 0) + 1, ppp_registration_row{});
    const int rc = ppp_register_mesh_tiles(hs.data(), ms.data(), hs.size(), &rp, T0, rows ? rows->data() : nullptr, rows ? rows->size() : 0, &st);
    if (rc != PPP_OK) {
        if (rows) rows->clear();
        const ppp_handle at = hs[st.failed_tile >= 0 ? (size_t)st.failed_tile : 0];
        std::fprintf(stderr, "ppp error %d: tile %d: %s\n", rc, st.failed_tile, at ? ppp_last_error(at) : "no handle");
        return false;
    }
    if (rows) rows->resize(std::min(rows->size(), (size_t)st.reg.steps + 1));
    return true;
}

} // namespace ppp
#endif
