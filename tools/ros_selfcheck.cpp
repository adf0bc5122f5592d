// tools/ros_selfcheck.cpp -- the closing procedure for the rows whose oracle restates UN-VENDORED third-party code
// ("missing" #3; the third row came with the VoxelGrid pre-filter):
//
//   f2  gem_show     restates grid_map's iteration order (GridMapIterator over the circular buffer), getPosition and the
//                    grid_map::Matrix layout that ElevationMap::show fills (reference: elevation_mapping/src/ElevationMap.cpp:85-149)
//   f4  gem_colorize restates OpenCV's cv::circle(img, p, 1, colour) as "the four edge neighbours of p", drawn into the image the later
//                    points sample (reference: elevation_mapping/src/ElevationMapping.cpp:349-381)
//   vox gem_voxel_device restates pcl::VoxelGrid<pcl::PCLPointCloud2> as pcl_ros's nodelet runs it (the launch files' filter stages);
//                    tests/voxel_ref.py restates the same contract in numpy
//   glob gem_global_loop_closure restates pcl::transformPointCloud (x' = x*m00 + (y*m01 + (z*m02 + m03)) in float, no FMA: the SSE2
//                    form of PCL >= 1.10 on x86-64) and KdTreeFLANN<PointXY>::radiusSearch (d2 < r2 strictly, sorted by d2, ties by
//                    index) as updateGlobalMap calls them (reference: elevation_mapping/src/ElevationMapping.cpp:790-840);
//                    tests/global_ref.py restates the same contract in numpy
//   sor gem_local_compose restates pcl::StatisticalOutlierRemoval<Anypoint> (setMeanK(20), setStddevMulThresh(1.0)) as
//                    pointCloudtoOctomap runs it on the grid cloud of prevMap_ (reference: elevation_mapping/src/ElevationMapping.cpp:
//                    1146-1156); tests/compose_ref.py restates the same contract in numpy.  Two details of that statement are decided
//                    by this row and by nothing else: which sqrt overload PCL's `sqrt(nn_dists[k])` resolves to (the row prints which
//                    value of gem_compose_params::flags matches) and that the product in sq_sum is a float product
//   cost gem_costmap_* restates costmap_2d (ROS noetic costmap_2d.cpp / costmap_layer.cpp) as the reference's two layers call it
//                    (layers/src/pointMap_layer.cpp:45-100, elevationMap_layer.cpp:42-87): worldToMap, getIndex, getSizeInMetersX / Y,
//                    updateOrigin, resetMaps, touch, updateWithOverwrite, updateWithMax; tests/costmap_ref.py restates the same
//                    contract in numpy.  The row drives the real Costmap2D / CostmapLayer calls through PointMapLayer's loop, a rolling
//                    trajectory and both combination rules, and compares every byte, origin and bound
//   octo gem_octree_build restates octomap::ColorOcTree (octomap 1.8 / 1.9: updateNode, integrateNodeColor, pruneNode, expandNode,
//                    updateInnerOccupancy, writeData behind octomap_msgs::fullMapToMsg) as pointCloudtoOctomap calls it (reference:
//                    elevation_mapping/src/ElevationMapping.cpp:1158-1173); tests/octree_ref.py restates the same contract in Python.
//                    The row inserts seeded clouds that prune and expand (rounds over full 2^3, 4^3 and 8^3 blocks of leaves merged
//                    with scattered points) into a real ColorOcTree and compares the stream byte for byte; it settles the five points
//                    include/gem_hip.h lists as not verified (prune on value only and the pruned node's colour, the host's exp, no
//                    contraction in the blend, the uint8_t cast, the empty tree)
//   foot gem_costmap_clear_footprint / gem_costmap_footprint_cost restate costmap_2d::transformFootprint (footprint.cpp),
//                    Costmap2D::setConvexPolygonCost (polygonOutlineCells + convexFillCells over the line iterator) and
//                    base_local_planner::CostmapModel::footprintCost (include/gem_hip_footprint.h; tests/footprint_ref.py restates the
//                    same contract in numpy).  The row clears seeded poses of the launch files' rectangle and of a 16-gon out of a real
//                    Costmap2D and scores seeded poses with a real CostmapModel on a noise grid, and compares every byte and every cost.
//                    The poses' cosines and sines are this host's std::cos / std::sin, as transformFootprint's are
//   mapgrid gem_costmap_mapgrid_prepare / _read restate base_local_planner::MapGrid (map_grid.cpp: adjustPlanResolution, setTargetCells,
//                    setLocalGoal, computeTargetDistance, updatePathCell; include/gem_hip_mapgrid.h; tests/mapgrid_ref.py restates the
//                    same contract in numpy).  The row runs a real MapGrid's setTargetCells and setLocalGoal over seeded plans that
//                    start off the map, cross noise grids with 253 / 254 / 255 cells and leave them again, and compares every
//                    target_dist of both grids.  MapGridCostFunction::scoreTrajectory is not driven (it needs a Trajectory and the
//                    planner's parameters): the scoring loop stays pinned on tests/mapgrid_ref.py alone
//   critics gem_critics_select restates base_local_planner::SimpleScoredSamplingPlanner (simple_scored_sampling_planner.cpp:
//                    scoreTrajectory with its early exit, findBestTrajectory; include/gem_hip_critics.h; tests/critics_ref.py restates the
//                    same contract in plain Python).  The row feeds a real planner seeded score tables through a table-driven
//                    TrajectoryCostFunction and a generator that numbers its trajectories, and compares the winner's index and cost.
//                    The critics' own scores are the foot and mapgrid rows'; ObstacleCostFunction and MapGridCostFunction are not driven
//   trajgen gem_trajgen_plan / gem_trajgen_generate restate base_local_planner::SimpleTrajectoryGenerator (simple_trajectory_generator.cpp:
//                    initialise, generateTrajectory, computeNewVelocities; velocity_iterator.h; include/gem_hip_trajgen.h;
//                    tests/trajgen_ref.py restates the same contract in plain Python).  The row drives a real generator over seeded
//                    states with and without use_dwa, by time and by distance, and compares, sample by sample: whether it was
//                    generated, the number of points, every (x, y, theta) as float bits -- x and y within num_steps ulps when the
//                    cos overload the library picks is not the double one, which the row reports FIRST and on its own -- and
//                    (xv, yv, thetav).  It also reports the deviation the header names: hypot against sqrt(x * x + y * y).
//                    OscillationCostFunction and TwirlingCostFunction are not driven (they need the planner's state); their rules
//                    are two lines each
//   navplan gem_costmap_navplan / _read restate global_planner (GlobalPlanner::makePlan with use_dijkstra, use_quadratic = false,
//                    use_grid_path: DijkstraExpansion::calculatePotentials over PotentialCalculator, Expander::getCost through
//                    gem_navplan_weights, GridPath::getPath; include/gem_hip_navplan.h, restated FROM MEMORY; tests/navplan_ref.py
//                    restates the same contract in numpy / plain Python).  The row drives the library's expansion and path objects
//                    over seeded noise grids whose rim it closes itself (outlineMap) and compares the goal's potential, the
//                    potential of every cell the library settled below the goal's (the library leaves at the goal, the device
//                    converges everywhere) and the path cell by cell.  convert_offset_ is makePlan's and is not driven.  It
//                    cannot be run where the test suite runs and has not been through a compiler
//   navquad gem_costmap_navplan_quadratic's increment (include/gem_hip_navquad.h) takes its three coefficients from
//                    global_planner::QuadraticCalculator::calculatePotential (the same as navfn's updateCell), RECALLED FROM MEMORY.
//                    The contract is the project's own -- integers, a floor, the clamp to 1 .. hf -- so the row does not ask for
//                    equality: over every hf in 1 .. 252 and every dc in 0 .. hf it feeds the library's calculator a 3 x 3 potential
//                    with ta and tc as two neighbours and compares its result with ta + inc(hf, dc) within the departures the
//                    header names (under one unit for the floor, 0.46 % of hf for the clamp, one unit where max(1, .) acts).  A
//                    wrong coefficient shows at once.  It has not been through a compiler either
//   obs  gem_costmap_observe restates costmap_2d::ObstacleLayer::updateBounds (obstacle_layer.cpp: raytraceFreespace with its four
//                    clips, updateRaytraceBounds, the marking loop), Costmap2D::raytraceLine / bresenham2D / cellDistance
//                    (costmap_2d.h) and the height window of ObservationBuffer::bufferCloud (include/gem_hip_obstacle.h;
//                    tests/obstacle_ref.py restates the same contract in numpy).  The row drives a real ObstacleLayer that was never
//                    initialised through ROS: its map is sized by hand, rolling and footprint clearing are off, and the observations
//                    are handed over by addStaticObservation, so updateBounds runs its own clearing and marking loops over seeded
//                    clouds that leave the map on every side, from sensors on and off the map, at two raytrace ranges.  Every byte
//                    and the four bounds are compared.  The height window is applied by the row while it builds the PointCloud2 (the
//                    buffer needs TF).  It also reports the deviations the header names: hypot against sqrt(x * x + y * y), in the
//                    integer form of raytraceLine and the double form of updateRaytraceBounds.  It cannot be compiled where the test
//                    suite runs and has not been through a compiler
//   voxel gem_costmap_voxel_observe restates costmap_2d::VoxelLayer::updateBounds (voxel_layer.cpp: raytraceFreespace with the
//                    2 * resolution shortening, its ceiling / floor clip and four edge clips, the marking loop, resetMaps,
//                    updateOrigin) and voxel_grid::VoxelGrid (voxel_grid.h: markVoxelInMap, clearVoxelLineInMap, raytraceLine,
//                    bresenham3D, bitsBelowThreshold), from memory (include/gem_hip_voxlayer.h; tests/voxlayer_ref.py restates the same
//                    contract in numpy, literally and as a set function).  THIS ROW IS TEXT ONLY: no code below drives it yet.  What
//                    it has to do, in the obs row's manner: a real VoxelLayer sized by hand (matchSize builds its voxel_grid_),
//                    rolling, footprint clearing and both publishers off, unknown_threshold_ / mark_threshold_ / z_resolution_ /
//                    origin_z_ / size_z_ set directly, the observations handed over by addStaticObservation; compare every byte of
//                    the costmap, every column of getVoxelGrid().getData() and the four bounds after updateBounds, with
//                    mark_threshold 0 (where the bounds must be equal) and 2 (where the header's named departure allows the device's
//                    to contain the library's).  It settles the header's open points: the popcount <= threshold reading of
//                    bitsBelowThreshold, no touch of the sensor, getSizeInMetersX for map_end, the 2 * resolution shortening, and
//                    sqrt against hypot
//   rollout gem_rollout_plan / gem_rollout_host / gem_rollout_pick restate base_local_planner::TrajectoryPlanner (trajectory_planner.cpp:
//                    createTrajectories, generateTrajectory, computeNewXPosition / YPosition / ThetaPosition,
//                    computeNewVelocity, footprintCost; trajectory_inc.h), from memory (include/gem_hip_rollout.h; tests/rollout_ref.py
//                    restates the same contract in plain Python, literally and as evaluate-all-then-pick).  THIS ROW IS TEXT ONLY: no
//                    code below drives it yet, and it cannot be compiled where the test suite runs.  What it has to do, in the
//                    trajgen row's manner: a real TrajectoryPlanner over a CostmapModel and a Costmap2D filled from seeded noise
//                    with a cleared block, heading_scoring, simple_attractor and meter_scoring off, dwa on and off, holonomic on
//                    and off, updatePlan with a plan across the map and findBestPath for seeded states -- it prepares path_map_
//                    and goal_map_ itself and calls createTrajectories -- against gem_costmap_mapgrid_prepare's grids read back
//                    and gem_rollout_host over them: the winner's (xv, yv, thetav) and cost bit for bit, its points through
//                    Trajectory::getPoint, and for the caller's flags a planner driven twice so that stuck_left_ / stuck_right_ and
//                    the strafe flags are set by its own bookkeeping.  It settles the header's open points: the pairing of a
//                    negative vtheta_samp with stuck_left, `<=` in the in-place and strafe phases against `<` in the forward one,
//                    hypot against sqrt(x * x + y * y) in the window, and whether int(... + 0.5) of num_steps sees the double or a
//                    float; and beside them whether escaping removes the forward phase only and the backward trajectory's cost
//                    of -1.0 becomes 1.0
//
// None of these libraries exists in the build image, so oracle/gem_oracle_show.c and oracle/gem_oracle_color.c are pinned on hand-computed
// scenes only.  This program is what a maintainer runs ONCE inside a ROS workspace that has the real grid_map_core and OpenCV (and an
// MI355X with libgem_hip.so): it drives the real libraries through the same loops the reference runs and compares every output of the
// HIP path bit for bit.  Exit code 0 = every row pinned on the real third-party code; non-zero = first difference printed.
// The vox row is bit for bit in the output order, the count and every voxel of one or two points; in voxels of three or more points
// it allows a few ulps, because PCL's std::sort is not stable and may sum such a voxel in another order than input order.
//
//   g++ -std=c++17 -O1 tools/ros_selfcheck.cpp -Iinclude -I/opt/ros/$ROS_DISTRO/include $(pkg-config --cflags eigen3 opencv4 pcl_filters-1.8 pcl_kdtree-1.8 pcl_search-1.8) \
//       -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Lgem_amd/lib -lgem_hip -Wl,-rpath,$PWD/gem_amd/lib -L/opt/rocm/lib -lamdhip64 \
//       -L/opt/ros/$ROS_DISTRO/lib -lgrid_map_core -lcostmap_2d -llayers -lroscpp -lrosconsole -ltf2_ros $(pkg-config --libs opencv4 pcl_filters-1.8 pcl_kdtree-1.8 pcl_search-1.8) -o ros_selfcheck && ./ros_selfcheck [seed]
//
// It cannot be compiled where the test suite runs (no ROS, grid_map, costmap_2d, OpenCV or PCL there); the cost row was written
// there, against the library's public headers as documented, and has not been through a compiler; neither have the octo row
// (add -loctomap -loctomath to the link line), the foot row (add -lbase_local_planner), the mapgrid row, the critics row and the trajgen
// row (the same library; the critics row also needs base_local_planner/simple_scored_sampling_planner.h among the includes, the
// trajgen row base_local_planner/simple_trajectory_generator.h and base_local_planner/local_planner_limits.h).  The navplan row has not
// been through a compiler either, nor has the navquad row; they are the rows of another package, global_planner: add -lglobal_planner
// to the link line (its headers are among the includes below).  The obs row has not been through a compiler either (costmap_2d's obstacle_layer.h
// pulls in tf2_ros, message_filters and laser_geometry: add -llaser_geometry -lmessage_filters to the link line).
//
// It is NOT part of the product and is not built by gem_amd/build.py; nothing here is needed on the GPU box of the test suite.
// The sor row filters a point type of its own (SorPoint), which PCL's precompiled libraries do not hold.  The define is file-wide, so
// the vox and glob rows now instantiate VoxelGrid, transformPointCloud and KdTreeFLANN from PCL's headers as well, instead of linking
// the precompiled instantiations they used before: the same templates, compiled here.
#define PCL_NO_PRECOMPILE
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstdio>
#include <cfloat>
#include <cstring>
#include <random>
#include <vector>

#include <Eigen/Dense>
#include <grid_map_core/GridMap.hpp>
#include <grid_map_core/iterators/GridMapIterator.hpp>
#include <opencv2/core.hpp>
#include <opencv2/imgproc.hpp>
#include <hip/hip_runtime_api.h>
#include <pcl/PCLPointCloud2.h>
#include <pcl/conversions.h>
#include <pcl/filters/voxel_grid.h>
#include <pcl/common/transforms.h>
#include <pcl/kdtree/kdtree_flann.h>
#include <pcl/filters/statistical_outlier_removal.h>
#include <pcl/search/kdtree.h>
#include <pcl/point_types.h>
#include <costmap_2d/cost_values.h>
#include <costmap_2d/costmap_2d.h>
#include <costmap_2d/costmap_layer.h>
#include <costmap_2d/footprint.h>
#include <costmap_2d/obstacle_layer.h>
#include <costmap_2d/observation.h>
#include <sensor_msgs/PointCloud2.h>
#include <sensor_msgs/point_cloud2_iterator.h>
#include <base_local_planner/costmap_model.h>
#include <base_local_planner/map_grid.h>
#include <base_local_planner/simple_scored_sampling_planner.h>
#include <global_planner/dijkstra.h>
#include <global_planner/grid_path.h>
#include <global_planner/potential_calculator.h>
#include <global_planner/quadratic_calculator.h>
#include <geometry_msgs/PoseStamped.h>
#include <geometry_msgs/Point.h>
#include <octomap/ColorOcTree.h>
#include <sstream>

#include <limits>
#include <map>

#include "gem_hip.h"

// the sor row's point: the fields of the library's 32-byte record (PointXYZRGBICT) as a registered PCL point
struct SorPoint {
    PCL_ADD_POINT4D;
    PCL_ADD_RGB;
    float covariance, intensity, travers;
    EIGEN_MAKE_ALIGNED_OPERATOR_NEW
} EIGEN_ALIGN16;
POINT_CLOUD_REGISTER_POINT_STRUCT(SorPoint, (float, x, x)(float, y, y)(float, z, z)(float, rgb, rgb)(float, covariance, covariance)
                                            (float, intensity, intensity)(float, travers, travers))

namespace {

int g_failures = 0;

#define CHECK_GEM(call)                                                                                     \
    do {                                                                                                    \
        const int rc_ = (call);                                                                             \
        if (rc_ != 0) { std::fprintf(stderr, "%s failed: %d (%s)\n", #call, rc_, gem_last_error(h)); return 2; } \
    } while (0)

bool same_bits(float a, float b)
{
    if (std::isnan(a) && std::isnan(b)) return true;            // grid_map's NaN and ours need not share a payload
    uint32_t x, y;
    std::memcpy(&x, &a, 4); std::memcpy(&y, &b, 4);
    return x == y;
}

void report(const char* what, long long at, double got, double want)
{
    if (g_failures++ < 20) std::fprintf(stderr, "MISMATCH %s at %lld: gem %.9g, real library %.9g\n", what, at, got, want);
}

// ---- f2 ------------------------------------------------------------------------------------------------------------------------
// A seeded map with holes (elevation -10), cells without traversability (-10 and NaN), colours, a moved circular buffer; then the loop of
// ElevationMap::show on a REAL grid_map::GridMap with the same geometry, start index and position, against gem_show.
int check_show(uint32_t seed)
{
    const int L = 96;
    const float res = 0.1f;
    gem_map_config cfg{};
    cfg.length = L; cfg.resolution = res; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    // two moves: the start index leaves (0, 0) on both axes and the centre becomes a lattice point other than the origin
    float centre[2]; int start[2]; float shift[2];
    const float p1[3] = {1.37f, -0.82f, 0.4f}, p2[3] = {2.91f, 0.33f, 0.4f};
    CHECK_GEM(gem_move(h, p1, centre, start, shift));
    CHECK_GEM(gem_move(h, p2, centre, start, shift));

    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    const size_t cells = (size_t)L * L;
    std::vector<float> elev(cells), var(cells), rough(cells), slope(cells), trav(cells), inten(cells);
    std::vector<int> cr(cells), cg(cells), cb(cells);
    for (size_t i = 0; i < cells; ++i) {
        const float r = u01(rng);
        elev[i] = r < 0.25f ? -10.0f : 2.0f * u01(rng) - 1.0f;
        var[i] = 1e-4f + 1e-3f * u01(rng);
        rough[i] = u01(rng); slope[i] = u01(rng);
        const float t = u01(rng);
        trav[i] = t < 0.1f ? -10.0f : (t < 0.15f ? std::nanf("") : u01(rng));
        inten[i] = 255.0f * u01(rng);
        cr[i] = (int)(255.0f * u01(rng)); cg[i] = (int)(255.0f * u01(rng)); cb[i] = (int)(255.0f * u01(rng));
    }
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_ELEVATION, elev.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_VARIANCE, var.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_ROUGH, rough.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_SLOPE, slope.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_TRAVER, trav.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_INTENSITY, inten.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_COLOR_R, cr.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_COLOR_G, cg.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_COLOR_B, cb.data()));

    const double map_length = (double)L * (double)res, resolution = (double)res;
    const double pos[2] = {(double)centre[0], (double)centre[1]};
    std::vector<float> visual(9 * cells), pxyz(3 * cells);
    std::vector<unsigned char> prgb(3 * cells), img(3 * cells);
    int count = -1;
    CHECK_GEM(gem_show(h, map_length, resolution, pos, visual.data(), pxyz.data(), prgb.data(), &count, img.data()));

    // the real thing: visualMap_ as the reference sets it up (ElevationMap.cpp:44, 80, 172-177) and show()'s loop (:97-127)
    const char* names[9] = {"elevation", "variance", "rough", "slope", "traver", "color_r", "color_g", "color_b", "intensity"};
    grid_map::GridMap vm({names[0], names[1], names[2], names[3], names[4], names[5], names[6], names[7], names[8]});
    vm.setGeometry(grid_map::Length(map_length, map_length), resolution, grid_map::Position(0.0, 0.0));
    vm.setStartIndex(grid_map::Index(start[0], start[1]));
    vm.setPosition(grid_map::Position(pos[0], pos[1]));
    vm.clearAll();
    cv::Mat image(L, L, CV_8UC3, cv::Scalar(0, 0, 0));
    std::vector<float> rxyz; std::vector<unsigned char> rrgb;
    const grid_map::Index s0 = vm.getStartIndex();
    for (grid_map::GridMapIterator it(vm); !it.isPastEnd(); ++it) {
        const int ix = (*it)(0), iy = (*it)(1);
        const size_t idx = (size_t)ix * L + iy;
        if (elev[idx] != -10 && trav[idx] != -10 && !std::isnan(trav[idx])) {
            vm.at("elevation", *it) = elev[idx]; vm.at("variance", *it) = var[idx]; vm.at("rough", *it) = rough[idx];
            vm.at("slope", *it) = slope[idx]; vm.at("traver", *it) = trav[idx];
            vm.at("color_r", *it) = cr[idx]; vm.at("color_g", *it) = cg[idx]; vm.at("color_b", *it) = cb[idx];
            vm.at("intensity", *it) = inten[idx];
            grid_map::Position p;
            vm.getPosition(*it, p);
            rxyz.push_back((float)p.x()); rxyz.push_back((float)p.y()); rxyz.push_back(vm.at("elevation", *it));
            rrgb.push_back((unsigned char)vm.at("color_r", *it)); rrgb.push_back((unsigned char)vm.at("color_g", *it));
            rrgb.push_back((unsigned char)vm.at("color_b", *it));
            cv::Vec3b& px = image.at<cv::Vec3b>((ix + L - s0[0]) % L, (iy + L - s0[1]) % L);
            px[0] = (unsigned char)vm.at("color_b", *it); px[1] = (unsigned char)vm.at("color_g", *it); px[2] = (unsigned char)vm.at("color_r", *it);
        }
    }
    const int before = g_failures;
    if (count != (int)(rxyz.size() / 3)) report("show: number of points", 0, count, (double)(rxyz.size() / 3));
    for (size_t i = 0; i < rxyz.size() && i < (size_t)3 * (size_t)std::max(count, 0); ++i)
        if (!same_bits(pxyz[i], rxyz[i])) report("show: point cloud xyz (grid_map iteration order, getPosition)", (long long)i, pxyz[i], rxyz[i]);
    for (size_t i = 0; i < rrgb.size() && i < (size_t)3 * (size_t)std::max(count, 0); ++i)
        if (prgb[i] != rrgb[i]) report("show: point cloud rgb", (long long)i, prgb[i], rrgb[i]);
    for (int l = 0; l < 9; ++l) {
        const grid_map::Matrix& m = vm.get(names[l]);                  // Eigen column-major, BUFFER order: the message's layout
        const float* d = m.data();
        for (size_t i = 0; i < cells; ++i)
            if (!same_bits(visual[(size_t)l * cells + i], d[i])) report(names[l], (long long)i, visual[(size_t)l * cells + i], d[i]);
    }
    for (int r = 0; r < L; ++r)
        for (int c = 0; c < L; ++c)
            for (int k = 0; k < 3; ++k)
                if (img[((size_t)r * L + c) * 3 + k] != image.at<cv::Vec3b>(r, c)[k]) report("show: orthomosaic", (long long)(r * L + c) * 3 + k, img[((size_t)r * L + c) * 3 + k], image.at<cv::Vec3b>(r, c)[k]);
    std::printf("f2 gem_show vs grid_map %s: %d points, 9 layers of %zu cells, %d x %d image: %s\n", "(GridMapIterator, getPosition, Matrix layout)",
                count, cells, L, L, g_failures == before ? "IDENTICAL" : "DIFFERENT");
    gem_destroy(h);
    return 0;
}

// ---- f4 ------------------------------------------------------------------------------------------------------------------------
// A seeded BGR image and a cloud whose points crowd a small part of it (so that circles overlap later pixels), through the literal loop of
// ElevationMapping::Callback with the real cv::circle, against gem_colorize.
int check_colorize(uint32_t seed)
{
    const int W = 160, H = 120, N = 60000;
    gem_map_config cfg{};
    cfg.length = 64; cfg.resolution = 0.1f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    cv::Mat img(H, W, CV_8UC3);
    for (int r = 0; r < H; ++r)
        for (int c = 0; c < W; ++c) img.at<cv::Vec3b>(r, c) = cv::Vec3b((unsigned char)(rng() & 255), (unsigned char)(rng() & 255), (unsigned char)(rng() & 255));
    const cv::Mat img0 = img.clone();
    // a pinhole looking along +x of the lidar frame: u = fx * (-y / x) + cx, v = fy * (-z / x) + cy
    gem_camera cam{};
    const double fx = 90.0, fy = 90.0, cx = W / 2.0, cy = H / 2.0;
    const double P[12] = {cx, -fx, 0.0, 0.0,   cy, 0.0, -fy, 0.0,   1.0, 0.0, 0.0, 0.0};
    std::memcpy(cam.lidar_to_image, P, sizeof(P));
    cam.width = W; cam.height = H;
    std::vector<float> xyzi(4 * (size_t)N);
    for (int i = 0; i < N; ++i) {
        const float x = (u01(rng) < 0.03f ? -1.0f : 1.0f) * (2.0f + 6.0f * u01(rng));       // a few points behind the camera
        xyzi[4 * i + 0] = x; xyzi[4 * i + 1] = x * (1.4f * u01(rng) - 0.7f) * (u01(rng) < 0.5f ? 0.3f : 1.2f);
        xyzi[4 * i + 2] = x * (u01(rng) - 0.5f); xyzi[4 * i + 3] = 1.0f + 100.0f * u01(rng);
    }
    std::vector<float> gx = xyzi;
    std::vector<uint32_t> grgb((size_t)N);
    CHECK_GEM(gem_colorize(h, &cam, N, gx.data(), img0.data, (size_t)img0.step, grgb.data()));

    // the reference's loop (ElevationMapping.cpp:349-381), on Eigen doubles as there
    Eigen::MatrixXd P34(3, 4);                                         // dynamic-size like the reference's P_lidar2img: the same product kernel
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) P34(r, c) = P[4 * r + c];
    const int before = g_failures;
    for (int i = 0; i < N; ++i) {
        Eigen::Vector4d pl(xyzi[4 * i], xyzi[4 * i + 1], xyzi[4 * i + 2], 1.0);
        const Eigen::Vector3d pi = P34 * pl;
        const float px = pi.x() / pi.z(), py = pi.y() / pi.z();
        cv::Point mid;
        mid.x = px; mid.y = py;
        uint32_t want = 0; float want_i = xyzi[4 * i + 3];
        if (mid.x > 0 && mid.x < img.size().width && mid.y > 0 && mid.y < img.size().height && pi.z() > 0) {
            const int b = img.at<cv::Vec3b>(mid.y, mid.x)[0], g = img.at<cv::Vec3b>(mid.y, mid.x)[1], r = img.at<cv::Vec3b>(mid.y, mid.x)[2];
            cv::circle(img, mid, 1, cv::Scalar(b, g, r));
            want = ((uint32_t)r << 16) | ((uint32_t)g << 8) | (uint32_t)b;
        } else want_i = 0.0f;
        if (grgb[i] != want) report("colorize: rgb of point (cv::circle drawn by the earlier points)", i, grgb[i], want);
        if (!same_bits(gx[4 * i + 3], want_i)) report("colorize: intensity of point", i, gx[4 * i + 3], want_i);
    }
    std::printf("f4 gem_colorize vs the loop with cv::circle (radius 1): %d points into a %d x %d image: %s\n", N, W, H,
                g_failures == before ? "IDENTICAL" : "DIFFERENT");
    gem_destroy(h);
    return 0;
}

// ---- vox -----------------------------------------------------------------------------------------------------------------------
// Seeded clouds with NaN points and crowded voxels through the real pcl::VoxelGrid<pcl::PCLPointCloud2> (setLeafSize, setFilterFieldName,
// setFilterLimits, setFilterLimitsNegative as the nodelet sets them), against gem_voxel_device with the same stage.
int check_voxel_stage(gem_handle* h, std::mt19937& rng, float leaf, const char* field, int field_id, double lo, double hi, bool negative)
{
    const int N = 200000;
    std::normal_distribution<float> xy(0.0f, 12.0f), z(0.0f, 1.0f);
    std::uniform_real_distribution<float> u01(0.0f, 1.0f);
    pcl::PointCloud<pcl::PointXYZI> cloud;
    cloud.resize(N);
    cloud.is_dense = false;
    for (int i = 0; i < N; ++i) {
        pcl::PointXYZI& p = cloud.points[i];
        p.x = xy(rng); p.y = xy(rng); p.z = z(rng); p.intensity = 255.0f * u01(rng);
        if (u01(rng) < 0.2f) { p.x = std::round(p.x * 2.0f) / 2.0f; p.y = std::round(p.y * 2.0f) / 2.0f; }   // crowded voxels
        if (u01(rng) < 0.02f) p.y = std::numeric_limits<float>::quiet_NaN();
    }
    pcl::PCLPointCloud2::Ptr in(new pcl::PCLPointCloud2), out(new pcl::PCLPointCloud2);
    pcl::toPCLPointCloud2(cloud, *in);
    pcl::VoxelGrid<pcl::PCLPointCloud2> vg;
    vg.setInputCloud(in);
    vg.setLeafSize(leaf, leaf, leaf);
    vg.setFilterFieldName(field);
    if (field[0]) { vg.setFilterLimits(lo, hi); vg.setFilterLimitsNegative(negative); }
    vg.filter(*out);
    pcl::PointCloud<pcl::PointXYZI> want;
    pcl::fromPCLPointCloud2(*out, want);

    std::vector<float> xyzi(4 * (size_t)N);
    for (int i = 0; i < N; ++i) {
        const pcl::PointXYZI& p = cloud.points[i];
        xyzi[4 * i] = p.x; xyzi[4 * i + 1] = p.y; xyzi[4 * i + 2] = p.z; xyzi[4 * i + 3] = p.intensity;
    }
    gem_voxel_params vp{};
    vp.leaf[0] = vp.leaf[1] = vp.leaf[2] = leaf;
    vp.field = field_id; vp.limit_min = lo; vp.limit_max = hi; vp.limit_negative = negative ? 1 : 0;
    if (!field[0]) { vp.limit_min = -FLT_MAX; vp.limit_max = FLT_MAX; }
    void *d_in = nullptr, *d_out = nullptr, *d_cnt = nullptr;
    if (hipMalloc(&d_in, xyzi.size() * 4) != hipSuccess || hipMalloc(&d_out, xyzi.size() * 4) != hipSuccess || hipMalloc(&d_cnt, 4) != hipSuccess) return 2;
    if (hipMemcpy(d_in, xyzi.data(), xyzi.size() * 4, hipMemcpyHostToDevice) != hipSuccess) return 2;
    CHECK_GEM(gem_voxel_device(h, &vp, 1, N, d_in, nullptr, d_out, nullptr, d_cnt));
    CHECK_GEM(gem_synchronize(h));
    int m = 0;
    std::vector<float> got(xyzi.size());
    if (hipMemcpy(&m, d_cnt, 4, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(got.data(), d_out, got.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return 2;
    (void)hipFree(d_in); (void)hipFree(d_out); (void)hipFree(d_cnt);

    // points per voxel, by the contract's key (gem_hip.h), to know which voxels may differ in the last bits
    const int before = g_failures;
    if (m != (int)want.size()) report("voxel: centroid count", -1, m, (double)want.size());
    const int k = std::min(m, (int)want.size());
    auto ulps = [](float a, float b) { int32_t x, y; std::memcpy(&x, &a, 4); std::memcpy(&y, &b, 4); return std::abs((long long)x - (long long)y); };
    std::map<uint32_t, int> count;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    const float inv = 1.0f / leaf;
    auto passes = [&](const float* p, bool dbl) {
        if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) return false;
        if (!field[0]) return true;
        const float v = p[field_id - 1];
        if (dbl) return negative ? !((double)v < hi && (double)v > lo) : !((double)v > hi || (double)v < lo);
        return negative ? !(v < (float)hi && v > (float)lo) : !(v > (float)hi || v < (float)lo);
    };
    for (int i = 0; i < N; ++i)
        if (passes(&xyzi[4 * i], false))
            for (int c = 0; c < 3; ++c) { mn[c] = std::min(mn[c], xyzi[4 * i + c]); mx[c] = std::max(mx[c], xyzi[4 * i + c]); }
    int mb[3], div[3];
    for (int c = 0; c < 3; ++c) { mb[c] = (int)std::floor(mn[c] * inv); div[c] = (int)std::floor(mx[c] * inv) - mb[c] + 1; }
    std::vector<uint32_t> keys;
    for (int i = 0; i < N; ++i) {
        if (!passes(&xyzi[4 * i], true)) continue;
        uint32_t key = 0, mul = 1;
        for (int c = 0; c < 3; ++c) { key += (uint32_t)((int)std::floor(xyzi[4 * i + c] * inv) - mb[c]) * mul; mul *= (uint32_t)div[c]; }
        ++count[key];
    }
    std::vector<int> voxel_size;
    for (const auto& kv : count) voxel_size.push_back(kv.second);      // ascending key = output order
    int relaxed = 0;
    for (int i = 0; i < k; ++i) {
        const float w[4] = {want.points[i].x, want.points[i].y, want.points[i].z, want.points[i].intensity};
        const bool crowded = i < (int)voxel_size.size() && voxel_size[i] >= 3;
        for (int c = 0; c < 4; ++c) {
            if (same_bits(got[4 * i + c], w[c])) continue;
            if (crowded && ulps(got[4 * i + c], w[c]) <= 4) { ++relaxed; continue; }
            report("voxel: centroid component", 4ll * i + c, got[4 * i + c], w[c]);
        }
    }
    std::printf("vox gem_voxel_device vs pcl::VoxelGrid<PCLPointCloud2> (leaf %g, field '%s' [%g, %g]%s): %d centroids: %s (%d components "
                "within 4 ulps in voxels of >= 3 points)\n", leaf, field, lo, hi, negative ? " negative" : "", m,
                g_failures == before ? "IDENTICAL" : "DIFFERENT", relaxed);
    return 0;
}

int check_voxel(uint32_t seed)
{
    gem_map_config cfg{};
    cfg.length = 64; cfg.resolution = 0.1f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    std::mt19937 rng(seed);
    int rc = check_voxel_stage(h, rng, 0.1f, "x", GEM_VOXEL_FIELD_X, -10.0, 10.0, false);          // filter.launch
    if (!rc) rc = check_voxel_stage(h, rng, 0.2f, "z", GEM_VOXEL_FIELD_Z, -25.0, 25.0, false);      // a filter_kitti.launch stage
    if (!rc) rc = check_voxel_stage(h, rng, 0.25f, "y", GEM_VOXEL_FIELD_Y, -3.0, 0.1, true);
    if (!rc) rc = check_voxel_stage(h, rng, 0.3f, "", GEM_VOXEL_FIELD_NONE, 0.0, 0.0, false);
    gem_destroy(h);
    return rc;
}

// ---- glob ----------------------------------------------------------------------------------------------------------------------
// (a) seeded records, non-finite ones included, through the real pcl::transformPointCloud with the node's Matrix4f, against submap 1
//     of a loop closure whose centres are too far apart for any pair step (the transform alone);
// (b) centre sets with a centre exactly at the radius, tied distances and coincident centres through the real KdTreeFLANN::radiusSearch,
//     against the rule gem_global_loop_closure documents, and against the device: one record per submap, all on one key with variance
//     0.5, so every pair step fuses exactly once and the fused count is the sum of (list length - 1) over the lists longer than two.
std::vector<int> documented_list(const std::vector<float>& c, int n, int i, float radius)
{
    const float r2 = (float)((double)radius * (double)radius);
    std::vector<std::pair<float, int>> hits;
    for (int j = 0; j < n; ++j) {
        const float dx = c[2 * j] - c[2 * i], dy = c[2 * j + 1] - c[2 * i + 1];
        const float d2 = dx * dx + dy * dy;
        if (d2 < r2) hits.emplace_back(d2, j);
    }
    std::sort(hits.begin(), hits.end());
    std::vector<int> out;
    for (const auto& p : hits) out.push_back(p.second);
    return out;
}

struct Rec { float x, y, z, pad; uint8_t b, g, r, a; float covariance, intensity, travers; };
static_assert(sizeof(Rec) == 32, "PointXYZRGBICT");

int check_global(uint32_t seed)
{
    gem_map_config cfg{};
    cfg.length = 64; cfg.resolution = 0.05f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-30.0f, 30.0f), ang(-0.05f, 0.05f);
    // (a)
    const int N = 100000;
    std::vector<Rec> cloud(N);
    pcl::PointCloud<pcl::PointXYZ> in;
    in.resize(N);
    in.is_dense = true;
    for (int i = 0; i < N; ++i) {
        Rec r{};
        r.x = u(rng); r.y = u(rng); r.z = u(rng) * 0.1f; r.pad = 1.0f; r.covariance = 2.0f;
        if (i == 7) r.x = std::numeric_limits<float>::infinity();
        if (i == 11) r.y = std::numeric_limits<float>::quiet_NaN();
        cloud[i] = r;
        in[i].x = r.x; in[i].y = r.y; in[i].z = r.z;
    }
    Eigen::Isometry3f opt = Eigen::Isometry3f::Identity(), traj = Eigen::Isometry3f::Identity();
    opt.rotate(Eigen::AngleAxisf(ang(rng), Eigen::Vector3f::UnitZ())); opt.pretranslate(Eigen::Vector3f(u(rng), u(rng), 0.1f));
    traj.rotate(Eigen::AngleAxisf(ang(rng), Eigen::Vector3f::UnitZ())); traj.pretranslate(Eigen::Vector3f(u(rng), u(rng), -0.2f));
    const Eigen::Matrix4f M = (opt * traj.inverse()).matrix();
    pcl::PointCloud<pcl::PointXYZ> out;
    pcl::transformPointCloud(in, out, M);
    CHECK_GEM(gem_global_enable(h, 2 * N));
    int idx = 0;
    CHECK_GEM(gem_global_push(h, cloud.data(), 1, &idx));
    CHECK_GEM(gem_global_push(h, cloud.data(), N, &idx));
    std::vector<float> T(32, 0.0f);
    std::copy(M.data(), M.data() + 16, T.begin() + 16);
    const float far[4] = {0.0f, 0.0f, 1e6f, 0.0f};
    long long fused = 0, n = 0;
    CHECK_GEM(gem_global_loop_closure(h, 2, T.data(), far, 25.0f, 0.05, &fused));
    std::vector<Rec> got(N);
    CHECK_GEM(gem_global_export(h, 1, got.data(), N, &n));
    int bad = 0;
    for (int i = 0; i < N && bad < 5; ++i) {
        const float w[3] = {out[i].x, out[i].y, out[i].z}, g[3] = {got[i].x, got[i].y, got[i].z};
        for (int c = 0; c < 3; ++c)
            if (std::memcmp(&w[c], &g[c], 4) != 0 && !(std::isnan(w[c]) && std::isnan(g[c]))) {
                std::fprintf(stderr, "glob: transformPointCloud record %d coord %d: pcl %a device %a\n", i, c, w[c], g[c]);
                ++bad; ++g_failures;
            }
    }
    // (b)
    const std::vector<std::vector<float>> sets = {
        {0, 0, 3, 4, 0, 1, 1, 0, 0, -1, -1, 0, 2.5f, 2.5f},               // (3, 4): exactly at radius 5; four ties at 1
        {0, 0, 0, 0, 5, 0, 10, 0, 0, 0, -5, 0},                            // coincident centres
    };
    const float radii[2] = {5.0f, 7.0f};
    for (size_t si = 0; si < sets.size(); ++si) {
        const std::vector<float>& c = sets[si];
        const int S = (int)c.size() / 2;
        pcl::PointCloud<pcl::PointXY>::Ptr pts(new pcl::PointCloud<pcl::PointXY>());
        for (int j = 0; j < S; ++j) { pcl::PointXY p; p.x = c[2 * j]; p.y = c[2 * j + 1]; pts->push_back(p); }
        pcl::KdTreeFLANN<pcl::PointXY> kd;
        kd.setInputCloud(pts);
        long long want = 0;
        for (int i = 0; i < S; ++i) {
            std::vector<int> ids; std::vector<float> d2;
            kd.radiusSearch((*pts)[i], radii[si], ids, d2);
            const std::vector<int> doc = documented_list(c, S, i, radii[si]);
            if (ids != doc) {
                std::fprintf(stderr, "glob: set %zu centre %d: radiusSearch gives", si, i);
                for (int j : ids) std::fprintf(stderr, " %d", j);
                std::fprintf(stderr, ", the documented rule");
                for (int j : doc) std::fprintf(stderr, " %d", j);
                std::fprintf(stderr, "\n");
                ++g_failures;
            }
            if (ids.size() > 2) want += (long long)ids.size() - 1;
        }
        CHECK_GEM(gem_global_enable(h, 64));
        Rec one{};
        one.x = 0.01f; one.y = 0.01f; one.z = 1.0f; one.pad = 1.0f; one.covariance = 0.5f;
        for (int j = 0; j < S; ++j) CHECK_GEM(gem_global_push(h, &one, 1, &idx));
        std::vector<float> eye(16 * S, 0.0f);
        for (int j = 0; j < S; ++j) eye[16 * j] = eye[16 * j + 5] = eye[16 * j + 10] = eye[16 * j + 15] = 1.0f;
        CHECK_GEM(gem_global_loop_closure(h, S, eye.data(), c.data(), radii[si], 0.05, &fused));
        if (fused != want) { std::fprintf(stderr, "glob: set %zu: device fused %lld, radiusSearch's lists give %lld\n", si, fused, want); ++g_failures; }
    }
    gem_destroy(h);
    return 0;
}

// ---- sor -----------------------------------------------------------------------------------------------------------------------
// A rough 128 x 128 map with holes and spikes, captured and kept as the previous capture.  Its grid cloud goes through the real
// pcl::StatisticalOutlierRemoval (kept indices) and the real pcl::search::KdTree (the 21 nearest squared distances of every point,
// summed here in both sqrt forms).  Against them: gem_local_compose_distances for flags 0 and GEM_COMPOSE_SQRT_DOUBLE (every
// distance, bit for bit), and the kept set each flag value gives (distance <= threshold) against PCL's kept indices.  The row passes
// when the distances of both forms agree with the search and at least one flag value reproduces PCL's kept indices; it prints which.
int check_sor(uint32_t seed)
{
    const int L = 128, K = 20;
    gem_map_config cfg{};
    cfg.length = L; cfg.resolution = 0.05f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    std::mt19937 rng(seed);
    std::normal_distribution<float> rough(0.0f, 0.08f);
    std::uniform_real_distribution<float> u(0.0f, 1.0f);
    std::vector<float> elev(L * L), trav(L * L);
    for (int i = 0; i < L * L; ++i) {
        elev[i] = rough(rng);
        if (u(rng) < 0.002f) elev[i] += 1.5f;
        if (u(rng) < 0.1f) elev[i] = -10.0f;
        trav[i] = u(rng) - 0.2f;
    }
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_ELEVATION, elev.data()));
    CHECK_GEM(gem_set_layer(h, GEM_LAYER_TRAVER, trav.data()));
    CHECK_GEM(gem_local_enable(h, 1024));
    CHECK_GEM(gem_local_capture(h, 0.0, 0.0, nullptr));
    CHECK_GEM(gem_local_keep_previous(h));
    std::vector<Rec> grid(L * L);
    int n = 0;
    CHECK_GEM(gem_local_grid_cloud(h, grid.data(), &n));
    pcl::PointCloud<SorPoint>::Ptr cloud(new pcl::PointCloud<SorPoint>);
    cloud->resize(n);
    for (int i = 0; i < n; ++i) {
        SorPoint& p = (*cloud)[i];
        p.x = grid[i].x; p.y = grid[i].y; p.z = grid[i].z; p.travers = grid[i].travers;
    }
    cloud->is_dense = true;
    pcl::StatisticalOutlierRemoval<SorPoint> sor;
    sor.setInputCloud(cloud);
    sor.setMeanK(K);
    sor.setStddevMulThresh(1.0);
    std::vector<int> kept;
    sor.filter(kept);
    // the search itself, summed in both forms
    pcl::search::KdTree<SorPoint> tree;
    tree.setInputCloud(cloud);
    std::vector<float> want[2] = {std::vector<float>(n), std::vector<float>(n)};
    std::vector<int> nn(K + 1);
    std::vector<float> d2(K + 1);
    for (int i = 0; i < n; ++i) {
        if (tree.nearestKSearch((*cloud)[i], K + 1, nn, d2) != K + 1) { std::fprintf(stderr, "sor: point %d: fewer than %d neighbours\n", i, K + 1); return 2; }
        double sf = 0.0, sd = 0.0;
        for (int k = 1; k <= K; ++k) { sf += (double)sqrtf(d2[k]); sd += std::sqrt((double)d2[k]); }
        want[0][i] = (float)(sf / K); want[1][i] = (float)(sd / K);
    }
    bool matches[2] = {false, false};
    for (int f = 0; f < 2; ++f) {
        gem_compose_params p{};
        p.mean_k = K; p.stddev_mul = 1.0; p.travers_threshold = 0.0; p.flags = f ? GEM_COMPOSE_SQRT_DOUBLE : 0;
        std::vector<float> dist(L * L);
        int m = 0, counts[3] = {0, 0, 0};
        double thr = 0.0;
        CHECK_GEM(gem_local_compose_distances(h, &p, dist.data(), &m));
        CHECK_GEM(gem_local_compose(h, &p, nullptr, nullptr, counts, &thr));
        if (m != n) { std::fprintf(stderr, "sor: flags %d: %d distances for %d points\n", f, m, n); ++g_failures; continue; }
        for (int i = 0; i < n; ++i)
            if (std::memcmp(&dist[i], &want[f][i], 4) != 0) {
                std::fprintf(stderr, "sor: flags %d point %d: search gives %a, device %a\n", f, i, want[f][i], dist[i]);
                ++g_failures;
                break;
            }
        std::vector<int> dev_kept;
        for (int i = 0; i < n; ++i) if ((double)dist[i] <= thr) dev_kept.push_back(i);
        if ((int)dev_kept.size() != counts[0] + counts[1]) { std::fprintf(stderr, "sor: flags %d: kept %zu, road + obstacle %d\n", f, dev_kept.size(), counts[0] + counts[1]); ++g_failures; }
        matches[f] = dev_kept == kept;
        std::printf("sor: flags = %d (%s): threshold %.17g, kept %zu of %d, pcl kept %zu: %s\n", f, f ? "sqrt((double)d2)" : "(double)sqrtf(d2)", thr,
                    dev_kept.size(), n, kept.size(), matches[f] ? "the kept indices MATCH" : "the kept indices differ");
    }
    if (!matches[0] && !matches[1]) { std::fprintf(stderr, "sor: neither value of flags reproduces StatisticalOutlierRemoval's kept indices\n"); ++g_failures; }
    gem_destroy(h);
    return 0;
}

// ---- cost ----------------------------------------------------------------------------------------------------------------------
// The protected pieces of CostmapLayer the two layers use, made callable; no layered costmap behind it (matchSize is not used).
struct CostProbe : costmap_2d::CostmapLayer {
    CostProbe(unsigned sx, unsigned sy, double res, double ox, double oy, unsigned char def)
    {
        default_value_ = def;
        enabled_ = true;
        resizeMap(sx, sy, res, ox, oy);
    }
    using costmap_2d::CostmapLayer::touch;
    using costmap_2d::CostmapLayer::updateWithMax;
    using costmap_2d::CostmapLayer::updateWithOverwrite;
    void updateBounds(double, double, double, double*, double*, double*, double*) override {}
    void updateCosts(costmap_2d::Costmap2D&, int, int, int, int) override {}
    void reset() override {}
};

bool same_costmap(gem_handle* h, int id, costmap_2d::Costmap2D& real, const char* what)
{
    const unsigned sx = real.getSizeInCellsX(), sy = real.getSizeInCellsY();
    std::vector<unsigned char> got((size_t)sx * sy);
    gem_costmap_config c{};
    if (gem_costmap_read(h, id, 0, 0, (int)sx, (int)sy, got.data(), sx) != 0 || gem_costmap_geometry(h, id, &c) != 0) { ++g_failures; return false; }
    if (c.origin_x != real.getOriginX() || c.origin_y != real.getOriginY()) { report(what, -1, c.origin_x, real.getOriginX()); return false; }
    for (size_t i = 0; i < got.size(); ++i)
        if (got[i] != real.getCharMap()[i]) { report(what, (long long)i, got[i], real.getCharMap()[i]); return false; }
    return true;
}

// PointMapLayer::updateBounds' loop over seeded clouds (on and off the map, on its edges, NaN travers) on a real layer costmap, a
// rolling trajectory through updateOrigin with sub-cell, multi-cell and larger-than-map steps, then both combination rules onto a
// master that holds 0, 100, 254 and 255 -- against gem_costmap_mark_points / roll_to / merge / read.
int check_cost(uint32_t seed)
{
    gem_map_config cfg{};
    cfg.length = 32; cfg.resolution = 0.05f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    const unsigned sx = 75, sy = 40;
    const double res = 0.2, thresh = 0.5;
    CostProbe real(sx, sy, res, -7.25, 4.125, costmap_2d::NO_INFORMATION);
    gem_costmap_config cc{};
    cc.size_x = sx; cc.size_y = sy; cc.resolution = res; cc.origin_x = -7.25; cc.origin_y = 4.125; cc.default_value = costmap_2d::NO_INFORMATION;
    int id = -1, master_id = -1;
    CHECK_GEM(gem_costmap_create(h, &cc, &id));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    double robot_x = -7.25 + real.getSizeInMetersX() / 2, robot_y = 4.125 + real.getSizeInMetersY() / 2;
    const double steps[6] = {0.07, 0.2, 0.33, 1.7, 9.0, 40.0};
    for (int k = 0; k < 48; ++k) {
        const int dx = (k % 8 < 3) - (k % 8 > 4), dy = ((k + 2) % 8 < 3) - ((k + 2) % 8 > 4);
        robot_x += dx * steps[k % 6]; robot_y += dy * steps[(k + 1) % 6];
        real.updateOrigin(robot_x - real.getSizeInMetersX() / 2, robot_y - real.getSizeInMetersY() / 2);
        CHECK_GEM(gem_costmap_roll_to(h, id, robot_x, robot_y));
        if (!same_costmap(h, id, real, "cost: updateOrigin")) break;
        std::vector<Rec> cloud(4000);
        for (size_t i = 0; i < cloud.size(); ++i) {
            Rec& r = cloud[i];
            r.x = (float)(real.getOriginX() + (u(rng) * 1.2 - 0.1) * sx * res); r.y = (float)(real.getOriginY() + (u(rng) * 1.2 - 0.1) * sy * res);
            r.travers = (float)u(rng);
            if (i % 97 == 0) r.travers = 0.5f;
            if (i % 101 == 0) r.travers = std::numeric_limits<float>::quiet_NaN();
            if (i % 503 == 0) { r.x = (float)real.getOriginX(); r.y = (float)real.getOriginY(); }
        }
        double want[4] = {1e30, 1e30, -1e30, -1e30}, got[4] = {1e30, 1e30, -1e30, -1e30};
        for (const Rec& r : cloud) {                                     // pointMap_layer.cpp:55-81
            unsigned int mx, my;
            const double px = r.x, py = r.y;
            if (!real.worldToMap(px, py, mx, my)) continue;
            real.getCharMap()[real.getIndex(mx, my)] = r.travers > thresh ? costmap_2d::FREE_SPACE : costmap_2d::LETHAL_OBSTACLE;
            real.touch(px, py, &want[0], &want[1], &want[2], &want[3]);
        }
        CHECK_GEM(gem_costmap_mark_points(h, id, cloud.data(), (long long)cloud.size(), thresh, got));
        for (int b = 0; b < 4; ++b) if (got[b] != want[b]) report("cost: touch bounds", b, got[b], want[b]);
        if (!same_costmap(h, id, real, "cost: PointMapLayer::updateBounds")) break;
    }
    for (int mode = 0; mode < 2; ++mode) {
        costmap_2d::Costmap2D master(sx, sy, res, real.getOriginX(), real.getOriginY(), costmap_2d::FREE_SPACE);
        const unsigned char vals[4] = {0, 100, 254, 255};
        for (size_t i = 0; i < (size_t)sx * sy; ++i) master.getCharMap()[i] = vals[rng() % 4];
        cc.origin_x = real.getOriginX(); cc.origin_y = real.getOriginY(); cc.default_value = costmap_2d::FREE_SPACE;
        CHECK_GEM(gem_costmap_create(h, &cc, &master_id));
        CHECK_GEM(gem_costmap_write(h, master_id, 0, 0, (int)sx, (int)sy, master.getCharMap(), sx));
        if (mode == 0) real.updateWithOverwrite(master, 7, 3, 61, 33);
        else real.updateWithMax(master, 7, 3, 61, 33);
        CHECK_GEM(gem_costmap_merge(h, id, master_id, 7, 3, 61, 33, mode));
        same_costmap(h, master_id, master, mode ? "cost: updateWithMax" : "cost: updateWithOverwrite");
        CHECK_GEM(gem_costmap_destroy(h, master_id));
    }
    gem_destroy(h);
    return 0;
}

// ---- foot ----------------------------------------------------------------------------------------------------------------------
// Seeded poses over the map's box widened by a tenth (so vertices and centres fall off it), two footprints: setConvexPolygonCost on
// a real Costmap2D against gem_costmap_clear_footprint, CostmapModel::footprintCost against gem_costmap_footprint_cost.
int check_foot(uint32_t seed)
{
    gem_map_config cfg{};
    cfg.length = 32; cfg.resolution = 0.05f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    const unsigned sx = 130, sy = 90;
    const double res = 0.05, ox = -3.1, oy = 2.7;
    costmap_2d::Costmap2D real(sx, sy, res, ox, oy, costmap_2d::NO_INFORMATION);
    gem_costmap_config cc{};
    cc.size_x = sx; cc.size_y = sy; cc.resolution = res; cc.origin_x = ox; cc.origin_y = oy; cc.default_value = costmap_2d::NO_INFORMATION;
    int id = -1;
    CHECK_GEM(gem_costmap_create(h, &cc, &id));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<std::vector<double>> specs(2);
    specs[0] = {-0.64, -0.40, -0.64, 0.40, 0.64, 0.40, 0.64, -0.40};    // costmap_common_params_local.yaml:8
    for (int k = 0; k < 16; ++k) { specs[1].push_back(0.9 * std::cos(2 * M_PI * k / 16)); specs[1].push_back(0.9 * std::sin(2 * M_PI * k / 16)); }
    for (const std::vector<double>& spec : specs) {
        const int nv = (int)spec.size() / 2;
        std::vector<geometry_msgs::Point> fp(nv), oriented;
        for (int i = 0; i < nv; ++i) { fp[i].x = spec[2 * i]; fp[i].y = spec[2 * i + 1]; }
        // the noise grid of the tests: 0 .. 252, 0.4 % lethal, 0.4 % unknown, a few inscribed
        for (size_t i = 0; i < (size_t)sx * sy; ++i) {
            const double v = u(rng);
            real.getCharMap()[i] = v < 0.004 ? 254 : v < 0.008 ? 255 : v < 0.009 ? 253 : (unsigned char)(rng() % 253);
        }
        CHECK_GEM(gem_costmap_write(h, id, 0, 0, (int)sx, (int)sy, real.getCharMap(), sx));
        base_local_planner::CostmapModel model(real);
        const int n = 4000;
        std::vector<gem_footprint_pose> poses(n);
        std::vector<int> got(n);
        std::vector<double> want(n);
        for (int k = 0; k < n; ++k) {
            const double x = ox + (u(rng) * 1.2 - 0.1) * sx * res, y = oy + (u(rng) * 1.2 - 0.1) * sy * res, th = (u(rng) * 2 - 1) * M_PI;
            poses[k] = gem_footprint_pose{x, y, std::cos(th), std::sin(th)};
            costmap_2d::transformFootprint(x, y, th, fp, oriented);
            geometry_msgs::Point at; at.x = x; at.y = y;
            want[k] = model.footprintCost(at, oriented, 0.0, 0.0);
        }
        CHECK_GEM(gem_costmap_footprint_cost(h, id, poses.data(), n, spec.data(), nv, 0, got.data()));
        for (int k = 0; k < n; ++k) if ((double)got[k] != want[k]) report("foot: footprintCost", k, got[k], want[k]);
        // clearing: updateFootprint's transform and touch, then setConvexPolygonCost
        for (int k = 0; k < 200; ++k) {
            oriented.resize(nv);
            for (int i = 0; i < nv; ++i) {                                // transformFootprint's lines, from the pose's own cosine and sine
                oriented[i].x = poses[k].x + (fp[i].x * poses[k].cos_th - fp[i].y * poses[k].sin_th);
                oriented[i].y = poses[k].y + (fp[i].x * poses[k].sin_th + fp[i].y * poses[k].cos_th);
            }
            const bool want_ok = real.setConvexPolygonCost(oriented, costmap_2d::FREE_SPACE);
            int ok = -1;
            CHECK_GEM(gem_costmap_clear_footprint(h, id, &poses[k], spec.data(), nv, nullptr, &ok));
            if ((ok != 0) != want_ok) report("foot: setConvexPolygonCost's return", k, ok, want_ok);
            if (!same_costmap(h, id, real, "foot: setConvexPolygonCost")) break;
        }
    }
    gem_destroy(h);
    return 0;
}

// ---- obs -----------------------------------------------------------------------------------------------------------------------
// A real ObstacleLayer without ROS around it: the map sized by hand, everything updateBounds would ask a LayeredCostmap for switched off.
struct ObstacleProbe : costmap_2d::ObstacleLayer {
    ObstacleProbe(unsigned sx, unsigned sy, double res, double ox, double oy, double max_height)
    {
        resizeMap(sx, sy, res, ox, oy);
        default_value_ = costmap_2d::NO_INFORMATION;
        rolling_window_ = false; footprint_clearing_enabled_ = false; enabled_ = true; current_ = true;
        max_obstacle_height_ = max_height;
        combination_method_ = 1;
    }
};

int check_obs(uint32_t seed)
{
    gem_map_config cfg{};
    cfg.length = 32; cfg.resolution = 0.05f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    const unsigned sx = 130, sy = 90;
    const double res = 0.05, ox = -3.1, oy = 2.7, w = sx * res, hgt = sy * res, layer_max = 1.5, lo = 0.0, hi = 2.0;
    gem_costmap_config cc{};
    cc.size_x = sx; cc.size_y = sy; cc.resolution = res; cc.origin_x = ox; cc.origin_y = oy; cc.default_value = costmap_2d::NO_INFORMATION;
    int id = -1;
    CHECK_GEM(gem_costmap_create(h, &cc, &id));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    const double sensors[4][2] = {{ox + 0.37 * w, oy + 0.61 * hgt}, {ox + 0.3 * res, oy + 0.6 * res}, {ox + 20 * res, oy + 31 * res}, {ox - 0.05 * w, oy + 0.5 * hgt}};
    long long hypot_int = 0, hypot_double = 0;
    for (int k = 0; k < 8; ++k) {
        ObstacleProbe real(sx, sy, res, ox, oy, layer_max);
        for (size_t i = 0; i < (size_t)sx * sy; ++i) real.getCharMap()[i] = (unsigned char)(rng() % 253);
        CHECK_GEM(gem_costmap_write(h, id, 0, 0, (int)sx, (int)sy, real.getCharMap(), sx));
        const double sx0 = sensors[k % 4][0], sy0 = sensors[k % 4][1], sz0 = 0.8, raytrace = (k < 4 ? 0.4 : 2.0) * w, obstacle = 0.35 * w;
        const int n = 4000;
        std::vector<float> xyz;                                            // what the call reads: every record, the window applied by the library's twin below
        for (int i = 0; i < n; ++i) {
            xyz.push_back((float)(ox + (u(rng) * 1.6 - 0.3) * w)); xyz.push_back((float)(oy + (u(rng) * 1.6 - 0.3) * hgt)); xyz.push_back((float)(u(rng) * 3.0 - 0.5));
            if (i % 211 == 0) xyz[xyz.size() - 3] = (float)sx0;              // a == 0
            if (i % 223 == 0) xyz[xyz.size() - 2] = (float)sy0;              // b == 0
        }
        // ObservationBuffer::bufferCloud's height window, then the cloud as the buffer would hold it
        sensor_msgs::PointCloud2 cloud;
        sensor_msgs::PointCloud2Modifier mod(cloud);
        mod.setPointCloud2FieldsByString(1, "xyz");
        std::vector<int> kept;
        for (int i = 0; i < n; ++i) if ((double)xyz[3 * i + 2] <= hi && (double)xyz[3 * i + 2] >= lo) kept.push_back(i);
        mod.resize(kept.size());
        sensor_msgs::PointCloud2Iterator<float> ix(cloud, "x"), iy(cloud, "y"), iz(cloud, "z");
        for (int i : kept) { *ix = xyz[3 * i]; *iy = xyz[3 * i + 1]; *iz = xyz[3 * i + 2]; ++ix; ++iy; ++iz; }
        geometry_msgs::Point origin; origin.x = sx0; origin.y = sy0; origin.z = sz0;
        costmap_2d::Observation seen(origin, cloud, obstacle, raytrace);
        real.addStaticObservation(seen, true, true);
        double want[4] = {1e30, 1e30, -1e30, -1e30}, got[4] = {1e30, 1e30, -1e30, -1e30};
        real.updateBounds(0.0, 0.0, 0.0, &want[0], &want[1], &want[2], &want[3]);
        gem_observation o{};
        o.points = xyz.data(); o.n = n; o.point_step = 12; o.flags = GEM_OBS_MARKING | GEM_OBS_CLEARING;
        o.origin[0] = sx0; o.origin[1] = sy0; o.origin[2] = sz0; o.obstacle_range = obstacle; o.raytrace_range = raytrace;
        o.min_obstacle_height = lo; o.max_obstacle_height = hi;
        CHECK_GEM(gem_costmap_observe(h, id, &o, 1, layer_max, got));
        for (int b = 0; b < 4; ++b) if (got[b] != want[b]) report("obs: touch bounds", b, got[b], want[b]);
        if (!same_costmap(h, id, real, "obs: ObstacleLayer::updateBounds")) break;
        // the named deviations, counted: hypot against sqrt(x * x + y * y)
        for (int dx = -129; dx <= 129; dx += 1 + k) for (int dy = -89; dy <= 89; ++dy)
            hypot_int += std::hypot((double)dx, (double)dy) != std::sqrt((double)(dx * dx + dy * dy));
        for (int i = 0; i < n; ++i) {
            const double ddx = (double)xyz[3 * i] - sx0, ddy = (double)xyz[3 * i + 1] - sy0;
            hypot_double += std::hypot(ddx, ddy) != std::sqrt(ddx * ddx + ddy * ddy);
        }
    }
    std::printf("obs: hypot differs from sqrt(x * x + y * y) for %lld integer and %lld double arguments of those tried\n", hypot_int, hypot_double);
    gem_destroy(h);
    return 0;
}

// ---- mapgrid -------------------------------------------------------------------------------------------------------------------
// Seeded plans over noise grids: MapGrid::setTargetCells / setLocalGoal on a real Costmap2D against gem_costmap_mapgrid_prepare.
int check_mapgrid(uint32_t seed)
{
    gem_map_config cfg{};
    cfg.length = 32; cfg.resolution = 0.05f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    const unsigned sx = 130, sy = 90;
    const double res = 0.05, ox = -3.1, oy = 2.7;
    costmap_2d::Costmap2D real(sx, sy, res, ox, oy, costmap_2d::FREE_SPACE);
    gem_costmap_config cc{};
    cc.size_x = sx; cc.size_y = sy; cc.resolution = res; cc.origin_x = ox; cc.origin_y = oy; cc.default_value = costmap_2d::FREE_SPACE;
    int id = -1;
    CHECK_GEM(gem_costmap_create(h, &cc, &id));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    for (const double blocked : {0.0, 0.1, 0.3}) {
        for (size_t i = 0; i < (size_t)sx * sy; ++i) {
            const double v = u(rng);
            real.getCharMap()[i] = v < blocked ? (unsigned char)(253 + rng() % 3) : (unsigned char)(rng() % 253);
        }
        CHECK_GEM(gem_costmap_write(h, id, 0, 0, (int)sx, (int)sy, real.getCharMap(), sx));
        for (int k = 0; k < 20; ++k) {
            // three to six points over the map's box widened by a tenth: a plan may start off the map, leave it and come back
            std::vector<geometry_msgs::PoseStamped> plan(3 + rng() % 4);
            std::vector<double> xy;
            for (geometry_msgs::PoseStamped& p : plan) {
                p.pose.position.x = ox + (u(rng) * 1.2 - 0.1) * sx * res; p.pose.position.y = oy + (u(rng) * 1.2 - 0.1) * sy * res;
                p.pose.orientation.w = 1.0;
                xy.push_back(p.pose.position.x); xy.push_back(p.pose.position.y);
            }
            base_local_planner::MapGrid path(sx, sy), goal(sx, sy);
            path.resetPathDist(); goal.resetPathDist();
            path.setTargetCells(real, plan);
            goal.setLocalGoal(real, plan);
            CHECK_GEM(gem_costmap_mapgrid_prepare(h, id, xy.data(), (long long)plan.size(), GEM_MAPGRID_PATH | GEM_MAPGRID_GOAL));
            std::vector<int> got((size_t)sx * sy);
            for (int w = 0; w < 2; ++w) {
                int started = -1, cell[2];
                CHECK_GEM(gem_costmap_mapgrid_read(h, id, w ? GEM_MAPGRID_GOAL : GEM_MAPGRID_PATH, got.data(), &started, cell));
                base_local_planner::MapGrid& lib = w ? goal : path;
                long long differ = 0;
                for (unsigned y = 0; y < sy; ++y)
                    for (unsigned x = 0; x < sx; ++x) differ += (double)got[(size_t)y * sx + x] != lib(x, y).target_dist;
                if (differ) report(w ? "mapgrid: setLocalGoal, cells that differ" : "mapgrid: setTargetCells, cells that differ", k, (double)differ, 0.0);
            }
        }
    }
    gem_destroy(h);
    return 0;
}

// ---- critics -------------------------------------------------------------------------------------------------------------------
// Seeded score tables through a real SimpleScoredSamplingPlanner (its early exit included) against gem_critics_select.
struct TableGenerator : base_local_planner::TrajectorySampleGenerator {
    long long n = 0, next = 0;
    bool hasMoreTrajectories() override { return next < n; }
    bool nextTrajectory(base_local_planner::Trajectory& traj) override
    {
        traj.resetPoints();
        traj.xv_ = (double)next++;                                       // the trajectory's number travels in its velocity sample
        return true;
    }
};
struct TableCost : base_local_planner::TrajectoryCostFunction {
    const double* row = nullptr;
    bool prepare() override { return true; }
    double scoreTrajectory(base_local_planner::Trajectory& traj) override { return row[(long long)traj.xv_]; }
};

int check_critics(uint32_t seed)
{
    std::mt19937 rng(seed);
    for (int k = 0; k < 400; ++k) {
        const int nc = 1 + (int)(rng() % GEM_CRITIC_MAX);
        const long long nt = k % 40 == 7 ? 0 : 1 + (long long)(rng() % 200);
        std::vector<gem_critic> critics((size_t)nc);
        std::vector<double> scores((size_t)nc * (size_t)nt);
        for (int c = 0; c < nc; ++c) critics[(size_t)c] = gem_critic{GEM_CRITIC_EXTERNAL, 0, 0, c, (double)(rng() % 9) / 4.0, 0.0};
        for (double& v : scores) v = rng() % 10 == 0 ? -(double)(1 + rng() % 7) : (double)(rng() % 12) / 4.0;      // quarters: exact sums, many ties
        std::vector<TableCost> costs((size_t)nc);
        std::vector<base_local_planner::TrajectoryCostFunction*> list;
        for (int c = 0; c < nc; ++c) {
            costs[(size_t)c].row = scores.data() + (size_t)c * (size_t)nt;
            costs[(size_t)c].setScale(critics[(size_t)c].scale);
            list.push_back(&costs[(size_t)c]);
        }
        TableGenerator gen;
        gen.n = nt;
        std::vector<base_local_planner::TrajectorySampleGenerator*> gens{&gen};
        base_local_planner::SimpleScoredSamplingPlanner planner(gens, list);
        base_local_planner::Trajectory best;
        const bool found = planner.findBestTrajectory(best);
        gem_best_trajectory got{};
        CHECK_GEM(gem_critics_select(critics.data(), nc, scores.empty() ? nullptr : scores.data(), nt, nullptr, &got));
        if (found != (got.index >= 0)) report("critics: a winner was found by one side only", k, (double)got.index, (double)found);
        else if (found && ((long long)best.xv_ != got.index || best.cost_ != got.cost)) report("critics: the winner or its cost differs", k, got.cost, best.cost_);
    }
    return 0;
}

// ---- trajgen -------------------------------------------------------------------------------------------------------------------
// Seeded states through a real SimpleTrajectoryGenerator against gem_trajgen_plan / gem_trajgen_generate.  The contract promotes the
// float argument of the library's unqualified cos(pos[2]) to double; if the installed library picked the float overload, theta and
// the counts still agree and x / y drift by rounding: that case is told apart and reported as what it is.
int check_trajgen(uint32_t seed)
{
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    bool overload_reported = false;
    for (int k = 0; k < 200; ++k) {
        gem_trajgen_limits lim{0.3 + 0.5 * u(rng), k % 3 == 0 ? -0.2 : 0.0, 0.1 * (k % 2), -0.1 * (k % 2), 0.5 + u(rng), 0.4 * u(rng),
                               k % 5 == 0 ? -1.0 : 0.4 + 0.5 * u(rng), k % 7 == 0 ? -1.0 : 0.1 * u(rng), 1.0 + 2.0 * u(rng), 1.0 + 2.0 * u(rng), 1.0 + 3.0 * u(rng)};
        gem_trajgen_config cfg{1.0 + u(rng), 0.025 + 0.05 * u(rng), 0.05 + 0.1 * u(rng), 0.05 + 0.05 * u(rng), k % 4 != 0, (k / 4) % 2, k % 4 == 0, 0,
                               {1 + (int)(rng() % 8), 1 + (int)(rng() % 3), 1 + (int)(rng() % 12)}, 0};
        const float pos[3] = {(float)(10.0 * u(rng) - 5.0), (float)(10.0 * u(rng) - 5.0), (float)(6.28 * u(rng) - 3.14)};
        const float vel[3] = {(float)(lim.max_vel_x * u(rng)), (float)(0.05 * (k % 2) * (u(rng) - 0.5)), (float)(u(rng) - 0.5)};
        const float goal[2] = {pos[0] + (float)(3.0 * u(rng)), pos[1] + (float)(3.0 * u(rng) - 1.5)};
        base_local_planner::LocalPlannerLimits limits;
        limits.max_vel_x = lim.max_vel_x; limits.min_vel_x = lim.min_vel_x; limits.max_vel_y = lim.max_vel_y; limits.min_vel_y = lim.min_vel_y;
        limits.max_vel_theta = lim.max_vel_theta; limits.min_vel_theta = lim.min_vel_theta;
        limits.max_vel_trans = lim.max_vel_trans; limits.min_vel_trans = lim.min_vel_trans;
        limits.acc_lim_x = lim.acc_lim_x; limits.acc_lim_y = lim.acc_lim_y; limits.acc_lim_theta = lim.acc_lim_theta;
        base_local_planner::SimpleTrajectoryGenerator gen;
        gen.setParameters(cfg.sim_time, cfg.sim_granularity, cfg.angular_sim_granularity, cfg.use_dwa != 0, cfg.sim_period);
        gen.initialise(Eigen::Vector3f(pos[0], pos[1], pos[2]), Eigen::Vector3f(vel[0], vel[1], vel[2]), Eigen::Vector3f(goal[0], goal[1], 0.f), &limits,
                       Eigen::Vector3f((float)cfg.vsamples[0], (float)cfg.vsamples[1], (float)cfg.vsamples[2]), cfg.discretize_by_time != 0);
        gem_dwa_plan plan{};
        CHECK_GEM(gem_trajgen_plan(&lim, &cfg, pos, vel, goal, &plan));
        const int T = plan.max_steps > 0 ? plan.max_steps : 1;
        std::vector<gem_footprint_pose> poses((size_t)plan.n_traj * (size_t)T);
        std::vector<int> len((size_t)plan.n_traj);
        std::vector<double> ext(2 * (size_t)plan.n_traj);
        std::vector<float> v(3 * (size_t)plan.n_traj);
        CHECK_GEM(gem_trajgen_generate(&plan, pos, vel, poses.data(), len.data(), ext.data(), v.data(), T));
        long long t = 0;
        while (gen.hasMoreTrajectories()) {
            base_local_planner::Trajectory traj;
            const bool generated = gen.nextTrajectory(traj);
            if (t >= plan.n_traj) { report("trajgen: the library has more samples than the plan", k, (double)plan.n_traj, (double)t); break; }
            if (generated != (len[(size_t)t] > 0)) { report("trajgen: a sample was generated by one side only", k, (double)len[(size_t)t], (double)generated); ++t; continue; }
            if (generated) {
                if ((int)traj.getPointsSize() != len[(size_t)t]) report("trajgen: num_steps differs (hypot against sqrt, or ceil)", k, (double)len[(size_t)t], (double)traj.getPointsSize());
                else {
                    if ((float)traj.xv_ != v[3 * (size_t)t] || (float)traj.yv_ != v[3 * (size_t)t + 1] || (float)traj.thetav_ != v[3 * (size_t)t + 2])
                        report("trajgen: (xv, yv, thetav) differs", k, (double)v[3 * (size_t)t], traj.xv_);
                    for (int i = 0; i < len[(size_t)t]; ++i) {
                        double x, y, th;
                        traj.getPoint((unsigned)i, x, y, th);
                        const gem_footprint_pose& p = poses[(size_t)t * (size_t)T + (size_t)i];
                        if ((float)x != (float)p.x || (float)y != (float)p.y) {
                            const double ulp = std::ldexp(1.0, std::ilogb(std::fmax(std::fabs(x), std::fabs(p.x)) + 1e-30) - 23);
                            const bool drift = std::fabs(x - p.x) <= len[(size_t)t] * ulp + 1e-12;
                            if (drift && !overload_reported) {
                                std::printf("trajgen: x / y agree within num_steps float ulps but not to the bit: the library's cos(pos[2]) is NOT the double overload on a double-promoted argument (or its libm differs from the contract's cosine by more than its 2^-53)\n");
                                overload_reported = true;
                                ++g_failures;
                            } else if (!drift) report("trajgen: a pose differs", k, p.x, x);
                            break;
                        }
                    }
                }
            }
            ++t;
        }
        if (t != plan.n_traj) report("trajgen: the plan has more samples than the library", k, (double)plan.n_traj, (double)t);
    }
    return 0;
}

// ---- navplan -------------------------------------------------------------------------------------------------------------------
// Seeded noise grids through a real DijkstraExpansion + PotentialCalculator + GridPath against gem_costmap_navplan.  Written against
// the package's public headers as recalled; not compiled where the test suite runs.
int check_navplan(uint32_t seed)
{
    gem_map_config cfg{};
    cfg.length = 32; cfg.resolution = 0.05f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    const int sx = 130, sy = 90;
    const double res = 0.2, ox = -3.1, oy = 2.7;
    gem_costmap_config cc{};
    cc.size_x = sx; cc.size_y = sy; cc.resolution = res; cc.origin_x = ox; cc.origin_y = oy; cc.default_value = costmap_2d::FREE_SPACE;
    int id = -1;
    CHECK_GEM(gem_costmap_create(h, &cc, &id));
    int w[256];
    CHECK_GEM(gem_navplan_weights(50, 3.0, 253, 1, w));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(0.0, 1.0);
    std::vector<unsigned char> grid((size_t)sx * sy), outlined;
    for (const double noise : {0.0, 0.2, 0.3}) {
        for (unsigned char& b : grid) b = u(rng) < noise ? (unsigned char)(rng() % 256) : (unsigned char)0;
        CHECK_GEM(gem_costmap_write(h, id, 0, 0, sx, sy, grid.data(), sx));
        outlined = grid;                                                  // GlobalPlanner::outlineMap writes 254 into the rim; the device does not
        for (int x = 0; x < sx; ++x) outlined[x] = outlined[(size_t)(sy - 1) * sx + x] = costmap_2d::LETHAL_OBSTACLE;
        for (int y = 0; y < sy; ++y) outlined[(size_t)y * sx] = outlined[(size_t)y * sx + sx - 1] = costmap_2d::LETHAL_OBSTACLE;
        for (int k = 0; k < 10; ++k) {
            const int s[2] = {1 + (int)(rng() % (sx - 2)), 1 + (int)(rng() % (sy - 2))}, e[2] = {1 + (int)(rng() % (sx - 2)), 1 + (int)(rng() % (sy - 2))};
            global_planner::PotentialCalculator calc(sx, sy);
            global_planner::DijkstraExpansion expansion(&calc, sx, sy);
            expansion.setPreciseStart(false);
            expansion.setLethalCost(253); expansion.setNeutralCost(50); expansion.setFactor(3.0); expansion.setHasUnknown(true);
            std::vector<float> lib_pot((size_t)sx * sy);
            const bool lib_found = expansion.calculatePotentials(outlined.data(), s[0], s[1], e[0], e[1], sx * sy * 2, lib_pot.data());
            std::vector<std::pair<float, float>> lib_path;
            global_planner::GridPath walker(&calc);
            if (lib_found) walker.getPath(lib_pot.data(), s[0], s[1], e[0], e[1], lib_path);
            const double sxy[2] = {ox + (s[0] + 0.5) * res, oy + (s[1] + 0.5) * res}, exy[2] = {ox + (e[0] + 0.5) * res, oy + (e[1] + 0.5) * res};
            gem_navplan_status st{};
            CHECK_GEM(gem_costmap_navplan(h, id, sxy, exy, w, GEM_NAV_OUTLINE, nullptr, 0, &st));
            std::vector<int> pot((size_t)sx * sy), cells((size_t)st.n_path);
            CHECK_GEM(gem_costmap_navplan_read(h, id, pot.data(), cells.empty() ? nullptr : cells.data(), (long long)cells.size()));
            if ((st.found != 0) != lib_found) { report("navplan: found differs", k, (double)st.found, (double)lib_found); continue; }
            if (!lib_found) continue;
            const float goal_pot = lib_pot[(size_t)e[1] * sx + e[0]];
            if ((double)goal_pot != (double)st.goal_potential) report("navplan: the goal's potential differs", k, (double)st.goal_potential, goal_pot);
            long long differ = 0;                                         // the cells the library settled before it left at the goal
            for (size_t i = 0; i < pot.size(); ++i) differ += lib_pot[i] < goal_pot && (double)lib_pot[i] != (double)pot[i];
            if (differ) report("navplan: potentials below the goal's that differ", k, (double)differ, 0.0);
            // the library's path runs goal -> start before makePlan reverses it; the device's runs start -> goal
            if (lib_path.size() != cells.size()) { report("navplan: the path's length differs", k, (double)cells.size(), (double)lib_path.size()); continue; }
            for (size_t i = 0; i < cells.size(); ++i) {
                const std::pair<float, float>& p = lib_path[lib_path.size() - 1 - i];
                if ((int)p.first != cells[i] % sx || (int)p.second != cells[i] / sx) { report("navplan: a path cell differs", k, (double)cells[i], p.second * sx + p.first); break; }
            }
        }
    }
    gem_destroy(h);
    return 0;
}

// ---- navquad -------------------------------------------------------------------------------------------------------------------
// The library's quadratic update against the increment of include/gem_hip_navquad.h, through gem_navquad_host on a 3 x 3 map whose
// centre has the two neighbours ta and tc: not equality (the contract is the project's own), the departures the header names.
int check_navquad()
{
    global_planner::QuadraticCalculator calc(3, 3);
    for (int hf = 1; hf <= 252; ++hf)
        for (int dc = 0; dc <= hf; ++dc) {
            const float ta = 1000.0f, tc = ta + (float)dc;
            const float high = 1.0e10f;                                       // the package's POT_HIGH
            float pot[9] = {high, high, high, ta, high, high, high, tc, high};   // left = ta, down = tc
            const float lib = calc.calculatePotential(pot, (unsigned char)hf, 4, -1.0f);
            // the contract's increment, in the integers the header states
            const long long num = -2301ll * dc * dc + 5307ll * dc * hf + 7040ll * hf * hf, den = 10000ll * hf;
            const long long inc = dc >= hf ? hf : std::max(1ll, std::min<long long>(hf, num / den));
            const double slack = 1.0 + 0.0046 * hf + 1e-3 * hf;              // floor, clamp, float rounding of the library's polynomial
            if (std::fabs((double)lib - (1000.0 + (double)inc)) > slack) report("navquad: the library's update is not within the named departures", hf * 1000 + dc, 1000.0 + (double)inc, lib);
        }
    return 0;
}

// ---- octo ----------------------------------------------------------------------------------------------------------------------
// fullMapToMsg (octomap_msgs/conversions.h): msg.data = the bytes tree.writeData(stream) writes.  An empty tree writes nothing there
// only if the library agrees with the deliberate difference of gem_hip.h; the row reports it.
bool same_octree(gem_handle* h, const std::vector<Rec>& cloud, double res, const char* what)
{
    octomap::ColorOcTree tree(res);
    tree.clear();
    for (const Rec& r : cloud) {                                         // ElevationMapping.cpp:1158-1170
        tree.updateNode(octomap::point3d(r.x, r.y, r.z), true);
        tree.integrateNodeColor(r.x, r.y, r.z, r.r, r.g, r.b);
    }
    tree.updateInnerOccupancy();
    std::stringstream ss;
    tree.writeData(ss);
    const std::string want = ss.str();
    gem_octree_params q{};
    q.resolution = res;
    gem_octree_stats st{};
    if (gem_octree_build(h, GEM_OCTREE_USER0, &q, cloud.data(), (long long)cloud.size(), &st) != 0) { ++g_failures; return false; }
    std::vector<char> got((size_t)st.bytes + 1);
    size_t n = 0;
    if (gem_octree_read(h, GEM_OCTREE_USER0, got.data(), got.size(), &n) != 0) { ++g_failures; return false; }
    const bool same = n == want.size() && std::memcmp(got.data(), want.data(), n) == 0;
    std::printf("octo: %s: %zu points, octomap %zu bytes (%zu nodes), device %zu bytes, pruned leaves %lld, blocks %lld / %lld / %lld: %s\n", what,
                cloud.size(), want.size(), tree.size(), n, st.pruned_leaves, st.coupled_blocks[0], st.coupled_blocks[1], st.coupled_blocks[2],
                same ? "equal" : "DIFFERENT");
    if (!same) ++g_failures;
    return same;
}

int check_octo(uint32_t seed)
{
    gem_map_config cfg{};
    cfg.length = 32; cfg.resolution = 0.05f; cfg.mahalanobis_threshold = 5.0f; cfg.variance_floor = 1e-4f; cfg.obstacle_threshold = 0.5f; cfg.device = -1;
    gem_handle* h = nullptr;
    CHECK_GEM(gem_create(&cfg, &h));
    std::mt19937 rng(seed);
    std::uniform_real_distribution<double> u(-4.0, 4.0);
    same_octree(h, {}, 0.1, "empty cloud");
    for (int levels = 1; levels <= 3; ++levels) {
        for (const double res : {0.2, 0.1}) {
            // `rounds` rounds over one aligned block of 8^levels leaves, every round in a new order (the block collapses at the end of
            // a round, the next round's first point expands it; from round 5 on the leaves are saturated), scattered points in between
            const int side = 1 << levels, rounds = 7;
            std::vector<Rec> cloud;
            std::vector<int> order(side * side * side);
            for (int r = 0; r < rounds; ++r) {
                for (size_t i = 0; i < order.size(); ++i) order[i] = (int)i;
                std::shuffle(order.begin(), order.end(), rng);
                for (int i : order) {
                    Rec p{};
                    p.x = (float)(((i % side) + 3 * side + 0.5) * res); p.y = (float)((((i / side) % side) - 5 * side + 0.5) * res);
                    p.z = (float)(((i / side / side) + 2 * side + 0.5) * res);
                    p.r = (uint8_t)rng(); p.g = (uint8_t)rng(); p.b = (uint8_t)rng();
                    if (rng() % 50 == 0) p.r = p.g = p.b = 255;          // a white point leaves the colour unset
                    cloud.push_back(p);
                    if (rng() % 4 == 0) { Rec e{}; e.x = (float)u(rng); e.y = (float)u(rng); e.z = (float)(0.1 * u(rng)); e.r = (uint8_t)rng(); e.g = (uint8_t)rng(); e.b = (uint8_t)rng(); cloud.push_back(e); }
                }
            }
            char what[64];
            std::snprintf(what, sizeof what, "block of %d^3 leaves, res %.1f", side, res);
            same_octree(h, cloud, res, what);
        }
    }
    gem_destroy(h);
    return 0;
}

}  // namespace

int main(int argc, char** argv)
{
    const uint32_t seed = argc > 1 ? (uint32_t)std::strtoul(argv[1], nullptr, 10) : 20260101u;
    int rc = check_show(seed);
    if (rc == 0) rc = check_colorize(seed + 1u);
    if (rc == 0) rc = check_voxel(seed + 2u);
    if (rc == 0) rc = check_global(seed + 3u);
    if (rc == 0) rc = check_sor(seed + 4u);
    if (rc == 0) rc = check_cost(seed + 5u);
    if (rc == 0) rc = check_octo(seed + 6u);
    if (rc == 0) rc = check_foot(seed + 7u);
    if (rc == 0) rc = check_mapgrid(seed + 8u);
    if (rc == 0) rc = check_critics(seed + 9u);
    if (rc == 0) rc = check_trajgen(seed + 10u);
    if (rc == 0) rc = check_navplan(seed + 11u);
    if (rc == 0) rc = check_navquad();
    if (rc == 0) rc = check_obs(seed + 12u);
    if (rc) return rc;
    if (g_failures) { std::fprintf(stderr, "%d difference(s): the restatement of grid_map / cv::circle / pcl::VoxelGrid / transformPointCloud / KdTreeFLANN / StatisticalOutlierRemoval / costmap_2d / base_local_planner / global_planner / octomap does NOT match this installation\n", g_failures); return 1; }
    std::printf("all thirteen rows pinned on the installed grid_map_core, OpenCV, PCL, costmap_2d, base_local_planner, global_planner and octomap (seed %u)\n", seed);
    return 0;
}
