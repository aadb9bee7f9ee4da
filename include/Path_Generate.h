/*
 * Path_Generate.h -- drop-in for the reference header of the same name (class path_generater,
 * :33-75), the planner ./main links (src/main.cpp, src/Path_Generation.cpp): brute-force pairing
 * (insert_point, Path_Generation.cpp:107-206) and the float walks of slicing_method (:282-321)
 * and Contact_Path_Generation (:689-755) including its dynamic adjustment (compute_transform,
 * Area2Cloud, compute_boundary, bisection, dynamic_adjust_path, :362-634; k = 10 neighbours,
 * depth 0.005, Adjust_Threshold 1, toolthickness 10 as in the reference header :71).
 * compute_coverage / get_coverage (:463-496, 757-771) run on the engine after the pass (ppp_get_coverage); drawpath only
 * colours the viewer's cloud (show() dumps it).
 */
#ifndef PATH_GENERATION
#define PATH_GENERATION

#include <algorithm>
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

class path_generater {
public:
    path_generater() {}
    path_generater(std::string cloud_name, double Radius) : toolRadius(Radius), file_name(cloud_name)
    {
        ppp_params &p = planner.config().params;
        p.tool_radius = Radius; p.pairing = PPP_PAIR_BRUTE; p.walk = PPP_WALK_V1_CONTACT; p.change_range = 1; /* always x1000, :28-30 */
        planner.open(cloud_name);
    }
    ~path_generater() {}

    /* Path_Generation.cpp:37-51: other_cloud (inserted nodes, blue :196-198) + the cloud with the paths in red (:724) */
    void show()
    {
        const unsigned char node_rgb[3] = {0, 0, 255}, path_rgb[3] = {255, 0, 0};
        planner.show_dump(node_rgb, path_rgb);
    }
    void voxel_down(const float x, const float y, const float z) { planner.voxel_down(x, y, z); } /* Path_Generation.cpp:53-59 */
    void trans2center() { planner.trans2center(); } /* Path_Generation.cpp:60-92 */
    void smooth() { planner.smooth_mls(15, 3, file_name, true); } /* Path_Generation.cpp:340-360 */
    void Set_kdtree() {}
    void estimate_normal() { planner.estimate_normal(); } /* Path_Generation.cpp:323-333 */
    const std::vector<float> &cloud_normals() const { return planner.cloud_normals(); } /* n x (nx ny nz curvature) */
    /* Path_Generation.cpp:757-771: yes / no counted by float ++ (saturating at 2^24 as the reference's do), rate in float: 0 / 0
       (-nan) when no contact pass has run */
    void get_coverage()
    {
        size_t n = 0, covered = 0;
        if (!planner.coverage(n, covered)) n = covered = 0;
        const size_t sat = (size_t)1 << 24;
        float yes = (float)std::min(covered, sat), no = (float)std::min(n - covered, sat), rate;
        rate = yes / (yes + no);
        printf("yes: %f, no: %f\n", yes, no);
        printf("coverage rate: %f\n", rate);
    }

    /* the same two lines for the paths the last pass ends with, whichever planner ran (ppp_get_path_coverage): after
       Contact_Path_Generation with the adjustment the adjusted paths only, where get_coverage() also counts the raw ones */
    void get_path_coverage() { planner.print_path_coverage(); }
    /* how evenly those paths cover: the largest and mean contact count, the points two or more slices touch (ppp_get_path_contacts) */
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
    void get_deviation(const path_generater &ref) { planner.print_deviation(ref.planner, ppp::Planner::deviation_params_env(), &deviation_target); }
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
    void register_to(const path_generater &ref) { planner.print_registration(ref.planner, ppp::Planner::registration_params_env()); }
    /* register_to() against the triangles of the STL file `stl` themselves (ppp_register_mesh): the exact closest
       point and the facet's own normal, no pitch; the same lines */
    void register_to_mesh(const std::string &stl) { planner.print_mesh_registration(stl, ppp::Planner::registration_params_env()); }
    /* register_to() with the trimmed loop (ppp_register_trimmed; keep from PPP_REGISTER_KEEP, 0.8 where it is not set): a line
       with the kept and the paired counts and the cut, then register_to()'s lines over the kept pairs */
    void register_trimmed_to(const path_generater &ref) { planner.print_registration(ref.planner, ppp::Planner::trimmed_registration_params_env()); }
    /* register_to() with the robust loop (ppp_register_robust; tune from PPP_REGISTER_TUNE, sigma_min from PPP_REGISTER_SIGMA_MIN,
       4.685 and 1e-4 mm where they are not set): a line with the used / paired counts, the median and sigma, then register_to()'s */
    void register_robust_to(const path_generater &ref) { planner.print_registration(ref.planner, ppp::Planner::robust_registration_params_env()); }
    /* register_to_mesh() with the robust loop (ppp_register_mesh_robust): the facets' exact geometry under
       register_robust_to()'s weights, tune and sigma_min from the same variables */
    void register_robust_to_mesh(const std::string &stl) { planner.print_mesh_robust_registration(stl, ppp::Planner::robust_registration_params_env()); }
    /* register_to_mesh() with the trimmed loop (ppp_register_mesh_trimmed): the facets' exact geometry under
       register_trimmed_to()'s cut, keep from PPP_REGISTER_KEEP (0.8 where it is not set); PPP_REGISTER_BORDER=reject drops the
       candidates whose closest point lies on the mesh's border: a line with the kept, the paired and the on-border counts and the cut */
    void register_trimmed_to_mesh(const std::string &stl) { planner.print_mesh_trimmed_registration(stl, ppp::Planner::mesh_trimmed_registration_params_env()); }
    void register_global_to(const path_generater &ref) { planner.print_global_registration(ref.planner, ppp::Planner::global_registration_params_env()); }
    /* register_global_to() against the triangles of the STL file `stl` themselves (ppp_register_mesh_global): the
       mesh's area frame against the scan's point frame, the coarse chains and the fine chain on the facets; no pitch, no normal field */
    void register_global_to_mesh(const std::string &stl) { planner.print_mesh_global_registration(stl, ppp::Planner::global_registration_params_env()); }
    /* what the contact model says about the workpiece itself, before or apart from any path: the points with a contact width,
       its smallest / mean / largest half width, the points narrower than the slice step (ppp_get_contact_field) */
    void get_contact_field() { planner.print_contact_field(); }
    /* where the planned paths leave the workpiece untouched: the uncovered points as connected regions, one line per region of
       PPP_GAPS_MIN points or more with its size, extent and centre (ppp_get_regions) */
    void get_gaps() { planner.print_gaps(); }

    std::vector<int> rangedX_index(int position) { return planner.rangedX_index(position); }
    std::map<double, std::vector<double>> insert_point(std::vector<int> indices, Eigen::Vector3f PlanePoint)
    {
        return planner.insert_point(indices, PlanePoint[0]);
    }
    /* Path_Generation.cpp:282-321: insert_point on every slice of the min+step/2 walk */
    void slicing_method() { run(PPP_WALK_V1_SLICING, 0, "use time: "); }
    /* Path_Generation.cpp:689-755: contact paths, each adjusted against its predecessor's boundary */
    void Contact_Path_Generation()
    {
        printf("Start Path Planning!\n");
        run(PPP_WALK_V1_CONTACT, 1, "Toal Using Time: ");
    }
    std::vector<Spline> &paths() { return Path_set; }

private:
    void run(int walk, int adjust, const char *label)
    {
        auto t0 = std::chrono::high_resolution_clock::now();
        ppp_params &p = planner.config().params;
        p.walk = walk;
        p.dynamic_adjustment = adjust;
        p.curvature_k = 10; p.depth = depth; p.adjust_threshold = Adjust_Threshold; p.toolthickness = toolthickness;
        if (!planner.apply_params() || !planner.gen_path()) return;
        Path_set.clear();
        int S = planner.num_slices();
        for (int s = 0; s < S; ++s) Path_set.emplace_back(planner.handle(), s);
        auto us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::high_resolution_clock::now() - t0).count();
        std::cout << label << us << std::endl;
        std::cout << "number of paths: " << S << std::endl;
        std::ofstream outputFile("output.csv", std::ios::app); /* Path_Generation.cpp:312-320 */
        if (outputFile.is_open()) outputFile << us << std::endl;
    }

    ppp::Planner planner;
    std::vector<double> deviation_target; /* get_deviation()'s target map; empty: a uniform target */
    double toolRadius = 15, depth = 0.005, Adjust_Threshold = 1, toolthickness = 10; /* Path_Generate.h:71 */
    std::vector<Spline> Path_set;
    std::string file_name;
};

#endif
