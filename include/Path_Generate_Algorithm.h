/*
 * Path_Generate_Algorithm.h -- drop-in for the reference header of the same name
 * (class SectPath :57-98, class path_generater :102-135), used by src/connect.cpp and
 * src/connect1.cpp.  Same public methods and constructor arguments; the arithmetic runs on the
 * MI355X through include/ppp_hip.h.  Differences a caller can observe:
 *   - show() opens no PCL viewer: with PPP_SHOW_PCD=<file> it writes the cloud the viewer would show (inserted nodes +
 *     the cloud with the paths painted on it, path_slicing_alg.cpp:69-80, 269-288) as a PointXYZRGB PCD, else a notice;
 *   - Dynamic_adjustment = true runs the curvature-driven re-spacing (path_dynamic_alg.cpp:77-306)
 *     on the GPU, RemoveOutlier = true the statistical outlier removal (path_slicing_alg.cpp:101-108),
 *     Smooth = true the moving-least-squares smoothing (path_slicing_alg.cpp:111-139);
 *     Alignment = true the PCA alignment (path_slicing_alg.cpp:82-99; eigenvector order as Eigen's EigenSolver
 *     leaves it);
 *   - conditions on which the reference aborts (GSL / FLANN) are reported on stderr instead.
 * Build connect1's single-direction walk with -DPPP_SDIR (it links dynamic_alg_sdir.cpp in the
 * reference, CMakeLists.txt:38-47).
 */
#ifndef PATH_CONNECT
#define PATH_CONNECT

#include <chrono>
#include <fstream>
#include <string>
#include <vector>
#include "Spline.h"
/* The reference's drivers write `cout << ... << endl` unqualified (src/main.cpp:10,16, src/connect.cpp:13,19,
   src/connect1.cpp:13,19, src/contour.cpp:13,19).  Upstream those names reach them through THIS header ->
   pcl/visualization/cloud_viewer.h -> VTK's vtkIOStream.h (`using std::cout; using std::endl; using std::cerr;` at global
   scope).  The drop-in header takes PCL and VTK away, so it supplies the same three names itself -- here, in the header
   the drivers include, not in ppp_planner.hpp / Spline.h, whose other includers get nothing at global scope
   (tests/test_host_logic.py::test_reference_drivers_compile_unchanged).  -DPPP_NO_GLOBAL_IOSTREAM_NAMES leaves them out. */
#ifndef PPP_NO_GLOBAL_IOSTREAM_NAMES
#include <iostream>
using std::cerr;
using std::cout;
using std::endl;
#endif

#ifndef HANDEYEx /* (include/contour_alg.h brings its own calibration and trim) */
#define HANDEYEx -0.764091
#define HANDEYEy 0.025886
#define HANDEYEz 0.663790
#define HANDEYErx -3.1270175
#define HANDEYEry -0.040124
#define HANDEYErz -1.6063578
#endif
#ifndef PPP_NODE_GB
#define PPP_NODE_GB 0 /* green / blue of the inserted nodes' colour: red (path_slicing_alg.cpp:228-230); contour_alg.h makes them white */
#endif
#ifndef PPP_GETPATH_TRIM
#define PPP_GETPATH_TRIM 10 /* path_translation_alg.cpp:158-159: dy = miny + 10 ... bigy - 10 */
#endif

/* Base class: equal spacing path + robot path (path_slicing_alg.cpp, path_translation_alg.cpp) */
class SectPath {
public:
    SectPath() {}
    SectPath(std::string configName, std::string CloudFileName) : cloud_name(CloudFileName)
    {
        read_config(configName);
        planner.config().params.walk = PPP_WALK_SECTPATH;
        init_common();
        planner.open(cloud_name);
        if (ifSmooth) smooth();         /* path_slicing_alg.cpp:27 */
        if (ifAlign) trans2center();    /* path_slicing_alg.cpp:28 */
        if (ifRemove) remove_outlier(); /* path_slicing_alg.cpp:29 */
    }
    virtual ~SectPath() {}

    /* path_slicing_alg.cpp:82-99: PCA alignment; getPath then goes back through the inverse (path_translation_alg.cpp:146-174) */
    void trans2center() { planner.trans2center(); }
    /* path_slicing_alg.cpp:111-139: pcl::MovingLeastSquares, order 3, radius 15, and the smooth_<name> side file */
    void smooth() { planner.smooth_mls(15, 3, cloud_name, ifChangeRange); }

    /* path_slicing_alg.cpp:101-108: pcl::StatisticalOutlierRemoval, 50 neighbours, 1 sigma, on the resident cloud */
    void remove_outlier() { planner.remove_outlier(50, 1.0); }

    /* path_slicing_alg.cpp:69-80: other_cloud (the inserted nodes, red -- white in contour_alg.cpp:228-230) + the cloud with
       the paths drawn on it (drawpath: red for SectPath::GenPath :315,326, blue for the derived planner, path_dynamic_alg.cpp:330,354) */
    void show()
    {
        const unsigned char node_rgb[3] = {255, PPP_NODE_GB, PPP_NODE_GB}, path_rgb[3] = {(unsigned char)(blue_paths ? 0 : 255), 0, (unsigned char)(blue_paths ? 255 : 0)};
        /* the derived planner also paints each boundary curve green before it adjusts a slice against it (path_dynamic_alg.cpp:320-322) */
        planner.show_dump(node_rgb, path_rgb, blue_paths && planner.config().params.dynamic_adjustment != 0);
    }
    /* path_slicing_alg.cpp:141-150: the whole-cloud normal field (the reference's GenPath and getPath call it themselves;
       here they evaluate normals only where getPath needs them, so this runs when the CALLER asks for the field) */
    void estimate_normal() { planner.estimate_normal(); }
    const std::vector<float> &cloud_normals() const { return planner.cloud_normals(); } /* n x (nx ny nz curvature) */
    virtual void GenPath()
    {
        printf("Start Path Planning!\n");
        auto startT = std::chrono::high_resolution_clock::now();
        if (!planner.gen_path()) return;
        build_path_set();
        auto duration = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - startT).count();
        printf("Toal Using Time: %ld \n", (long)duration);          /* path_slicing_alg.cpp:337-341 */
        printf("Number of paths: %d\n", (int)Path_set.size());
        printf("Number of Point Cloud: %ld\n", (long)planner.num_points());
    }
    void getPath()
    {
        /* Path_set.erase(begin) + pop_back (path_translation_alg.cpp:149-150) happen inside the engine */
        std::cout << "Path number is " << (Path_set.size() >= 2 ? Path_set.size() - 2 : 0) << std::endl;
        std::vector<float> wp;
        if (!planner.get_path(wp)) return;
        WayPointsList.assign(wp.size() / 6, std::vector<float>(6));
        for (size_t w = 0; w < WayPointsList.size(); ++w)
            for (int d = 0; d < 6; ++d) WayPointsList[w][d] = wp[6 * w + d];
    }
    const std::vector<std::vector<float>> &waypoints() const { return WayPointsList; }
    /* the coverage rate of the planned paths, in get_coverage's two lines (Path_Generation.cpp:766-770; the v2 planner keeps the
       same lines commented out, path_dynamic_alg.cpp:155-160): the contact model on every slice's final path (ppp_get_path_coverage) */
    void get_path_coverage() { planner.print_path_coverage(); }
    /* how evenly the planned paths cover: the largest and mean contact count over the covered points, and the points two or more
       slices touch (ppp_get_path_contacts) */
    void get_path_contacts() { planner.print_path_contacts(); }
    /* how much the planned paths take off and how evenly: touched points, path length, mean / min / max removal and cv with the
       Hertzian profile (ppp_get_path_removal) */
    void get_path_removal() { planner.print_path_removal(); }
    /* what a feed schedule could do about it: a dwell factor per sample towards a uniform removal -- the factors' range, the
       residual before and after, the time factor (ppp_get_path_dwell) */
    void get_path_dwell() { planner.print_path_dwell(deviation_target.empty() ? nullptr : &deviation_target); }
    /* a timed feed schedule for the WayPointsList (needs getPath()): the dwell factor, the feed under a cap and an acceleration
       limit and the time per waypoint -- the waypoints by what limits them, the feed's range, the duration; writes
       <pathFile>.feed: pathFile's columns, then t and feed (ppp_get_path_feed, ppp_write_feed_file) */
    void get_path_feed() { planner.print_path_feed((std::string(planner.path_file()) + ".feed").c_str(), deviation_target.empty() ? nullptr : &deviation_target); }
    /* where this planner's cloud, the scan, stands proud of the cloud of ref (the nominal part, or the scan before the process;
       both registered in one frame): the scan's points by status, the deviation's range, mean and rms, the proud points
       (ppp_get_deviation; max_dist, smooth_radius, allowance and gain from PPP_DEVIATION_MAXDIST, _SMOOTH, _ALLOWANCE, _GAIN).
       Needs no pass.  The target map is kept: get_path_dwell() and get_path_feed() after it steer the removal towards it */
    void get_deviation(const SectPath &ref) { planner.print_deviation(ref.planner, ppp::Planner::deviation_params_env(), &deviation_target); }
    /* get_deviation() against the triangles of the STL file `stl` themselves (ppp_get_mesh_deviation; PPP_TRIMESH_CELL,
       PPP_TRIMESH_ORIENT=viewpoint): the same lines, and the closest points by region */
    void get_mesh_deviation(const std::string &stl) { planner.print_mesh_deviation(stl, ppp::Planner::deviation_params_env(), &deviation_target); }
    /* get_mesh_deviation() with the signed distance (ppp_get_mesh_signed_deviation): the topology's counts, a warning where the
       mesh is not closed, the same lines from the signed distance, and the points by sign and flag */
    void get_mesh_signed_deviation(const std::string &stl) { planner.print_mesh_deviation(stl, ppp::Planner::deviation_params_env(), &deviation_target, true); }
    /* this planner's cloud, the scan, registered to the cloud of ref by point-to-plane ICP from the identity (ppp_register;
       max_dist, iterations and min_step from PPP_REGISTER_MAXDIST, _ITERATIONS, _MINSTEP): prints the pairs and the rms before
       and after, the steps, the locked unknowns and T, and moves the cloud by T when the loop converged (ppp_transform_cloud:
       plan again afterwards).  ICP needs a start within the basin: a fixturing error, not an unknown pose */
    void register_to(const SectPath &ref) { planner.print_registration(ref.planner, ppp::Planner::registration_params_env()); }
    /* register_to() against the triangles of the STL file `stl` themselves (ppp_register_mesh): the exact closest
       point and the facet's own normal, no pitch; the same lines */
    void register_to_mesh(const std::string &stl) { planner.print_mesh_registration(stl, ppp::Planner::registration_params_env()); }
    /* register_to() with the trimmed loop (ppp_register_trimmed; keep from PPP_REGISTER_KEEP, 0.8 where it is not set): a line
       with the kept and the paired counts and the cut, then register_to()'s lines over the kept pairs */
    void register_trimmed_to(const SectPath &ref) { planner.print_registration(ref.planner, ppp::Planner::trimmed_registration_params_env()); }
    /* register_to() with the robust loop (ppp_register_robust; tune from PPP_REGISTER_TUNE, sigma_min from PPP_REGISTER_SIGMA_MIN,
       4.685 and 1e-4 mm where they are not set): a line with the used / paired counts, the median and sigma, then register_to()'s */
    void register_robust_to(const SectPath &ref) { planner.print_registration(ref.planner, ppp::Planner::robust_registration_params_env()); }
    /* register_to_mesh() with the robust loop (ppp_register_mesh_robust): the facets' exact geometry under
       register_robust_to()'s weights, tune and sigma_min from the same variables */
    void register_robust_to_mesh(const std::string &stl) { planner.print_mesh_robust_registration(stl, ppp::Planner::robust_registration_params_env()); }
    /* register_to_mesh() with the trimmed loop (ppp_register_mesh_trimmed): the facets' exact geometry under
       register_trimmed_to()'s cut, keep from PPP_REGISTER_KEEP (0.8 where it is not set); PPP_REGISTER_BORDER=reject drops the
       candidates whose closest point lies on the mesh's border: a line with the kept, the paired and the on-border counts and the cut */
    void register_trimmed_to_mesh(const std::string &stl) { planner.print_mesh_trimmed_registration(stl, ppp::Planner::mesh_trimmed_registration_params_env()); }
    void register_global_to(const SectPath &ref) { planner.print_global_registration(ref.planner, ppp::Planner::global_registration_params_env()); }
    /* register_global_to() against the triangles of the STL file `stl` themselves (ppp_register_mesh_global): the
       mesh's area frame against the scan's point frame, the coarse chains and the fine chain on the facets; no pitch, no normal field */
    void register_global_to_mesh(const std::string &stl) { planner.print_mesh_global_registration(stl, ppp::Planner::global_registration_params_env()); }
    /* what the contact model says about the workpiece itself, before or apart from any path: the points with a contact width,
       its smallest / mean / largest half width, the points narrower than the slice step (ppp_get_contact_field) */
    void get_contact_field() { planner.print_contact_field(); }
    /* where the planned paths leave the workpiece untouched: the uncovered points as connected regions, one line per region of
       PPP_GAPS_MIN points or more with its size, extent and centre (ppp_get_regions) */
    void get_gaps() { planner.print_gaps(); }

protected:
    virtual void read_config(std::string filename)
    {
        ppp_read_config(filename.c_str(), &planner.config());
        ppp_config &c = planner.config();
        toolRadius = c.params.tool_radius; PathResolution = c.params.path_resolution; RPYres = c.params.rpy_resolution;
        EElen = c.params.ee_length; ifChangeRange = c.params.change_range; ifAlign = c.alignment; ifSmooth = c.smooth_cloud;
        ifRemove = c.remove_outlier; pathFile = c.path_file;
    }
    void init_common()
    {
        ppp_params &p = planner.config().params;
        p.pairing = PPP_PAIR_KD; p.trim = PPP_GETPATH_TRIM; p.drop_ends = 1; p.smooth = 1;
        const float he[6] = {(float)HANDEYEx, (float)HANDEYEy, (float)HANDEYEz, (float)HANDEYErx, (float)HANDEYEry, (float)HANDEYErz};
        for (int i = 0; i < 6; ++i) p.handeye[i] = he[i];
    }
    void build_path_set()
    {
        Path_set.clear();
        int S = planner.num_slices();
        for (int s = 0; s < S; ++s) Path_set.emplace_back(planner.handle(), s);
    }

    /* Path planning Alg. */
    std::vector<int> rangedX_index(int position) { return planner.rangedX_index(position); }
    MAP insert_point(std::vector<int> indices, Eigen::Vector3f PlanePoint) { return planner.insert_point(indices, PlanePoint[0]); }

    ppp::Planner planner;
    std::vector<double> deviation_target; /* get_deviation()'s target map; empty: a uniform target */
    double toolRadius = 12, PathResolution = 7, RPYres = 7;
    float EElen = 0.3f;
    bool ifAlign = false, ifSmooth = false, ifChangeRange = true, ifRemove = false;
    std::vector<Spline> Path_set;
    std::string cloud_name, pathFile;
    std::vector<std::vector<float>> WayPointsList;
    bool blue_paths = false;
};

/* Derived class of the reference: dynamic adjustment (path_dynamic_alg.cpp / dynamic_alg_sdir.cpp) */
class path_generater : public SectPath {
public:
    path_generater() {}
    path_generater(std::string configName, std::string CloudFileName)
    {
        cloud_name = CloudFileName;
        blue_paths = true;
        read_config(configName);
#ifdef PPP_SDIR
        planner.config().params.walk = PPP_WALK_SDIR_INT;   /* dynamic_alg_sdir.cpp:349-374 */
#else
        planner.config().params.walk = PPP_WALK_CENTER_INT; /* path_dynamic_alg.cpp:308-372 */
#endif
        init_common();
        planner.open(cloud_name);
        if (ifSmooth) smooth();         /* path_dynamic_alg.cpp:29 */
        if (ifAlign) trans2center();    /* path_dynamic_alg.cpp:30 */
        if (ifRemove) remove_outlier(); /* path_dynamic_alg.cpp:32 */
    }
    void GenPath() override
    {
        printf("Start Path Planning!\n");
        auto startT = std::chrono::high_resolution_clock::now();
        if (!planner.gen_path()) return;
        build_path_set();
        auto duration = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - startT).count();
        printf("Toal Using Time: %ld \n", (long)duration);          /* path_dynamic_alg.cpp:374-378 */
        printf("Number of Point Cloud: %ld\n", (long)planner.num_points());
        std::ofstream outputFile("output.csv", std::ios::app);      /* path_dynamic_alg.cpp:380-388 */
        if (!outputFile.is_open()) std::cerr << "cannot open output.csv" << std::endl;
        else outputFile << duration << std::endl;
    }
    typedef enum { left, right } Dir;

private:
    void read_config(std::string filename) override
    {
        SectPath::read_config(filename);
        ppp_config &c = planner.config();
        depth = c.depth; Adjust_Threshold = c.adjust_threshold; toolthickness = c.toolthickness; Adjust = c.dynamic_adjustment;
        /* path_dynamic_alg.cpp:337-372: with Adjust the slices left/right of the centre are re-fitted
           against the boundary of their inner neighbour (compute_boundary / dynamic_adjust_path) */
        c.params.dynamic_adjustment = Adjust ? 1 : 0;
    }
    double depth = 0.01, Adjust_Threshold = 1, toolthickness = 10;
    bool Adjust = false;
};

#endif
