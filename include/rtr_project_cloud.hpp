// rtr_project_cloud.hpp -- header-only C++ facade with the reference's ProjectCloud surface
// (reference: src/RTRenderer/include/project_cloud.h:11-19) over the C ABI of rtr.h.
//
// The reference's header hard-wires cv::Mat, cv::Matx44d, CameraCalibration and
// std::unordered_map<int, OctreeGrid::Block>.  None of OpenCV / glm is in this build image,
// so the facade is written against the *members the reference actually uses* and accepts any
// types that provide them -- the reference's own types satisfy every requirement, so
// `rtr::ProjectCloud` is a source-level drop-in for `::ProjectCloud` in
// example/render_trajectory/main.cpp:87-96 and cloudreader.cpp:233-246:
//   Grid        : iterable of pairs whose .second has .positions (elements with .x .y .z) and
//                 .colors (elements indexable [0..2])            (Octreegrid.h:16-21,162-180)
//   Calibration : getWidth(), getHeight(), getIntrinsicsMatrix()(r,c)   (CameraCalibration.h)
//   Extrinsics  : operator()(r,c) -> double, world->camera              (cv::Matx44d)
//   Image       : template ptr<T>() -> T*  (cv::Mat::ptr<uint8_t>() / ptr<float>()),
//                 caller-allocated CV_8UC3 / CV_32F of size W x H      (main.cpp:93-94)
// Return codes as in project_cloud.cu:268-312: 1 on success, -1 when both outputs are null.
// Unlike the reference (exit(1) on CUDA errors, project_cloud.cu:13-17) failures throw.
//
// Beyond the reference: computePointIds / visible_points (rtr.h section 6b) name the points a frame shows, by their
// index in the grid's flattened vertex order (the order the constructor uploads); construct with point_ids = true
// when the library may sort the cloud (its default upload policy does for unordered clouds).  setClipPlanes /
// setClipBox / clearClip (rtr.h section 6d) leave part of the cloud out of every later frame; setPointKeep / hidePoints /
// clearPointKeep (section 6e) hide any set of vertices, by the same indices (point_ids = true when the cloud may be sorted).
// appendPoints (section 2b) adds a grid (one registered scan) or raw float4 / uchar4 arrays behind the resident cloud
// without uploading it again; the indices of computePointIds, visible_points and hidePoints continue across appends --
// the appended vertices follow every vertex given so far, in the same flattened order.
// removePoints (section 2c) takes vertices out for good and renumbers the rest; commitPointKeep removes what the keep
// mask in force hides.  transformPoints (section 2d) moves a range of vertices (one re-registered scan) by an affine
// transform where they lie: indices, order and the keep mask stay.
// selectBox / selectPlanes / selectRect (section 6f) name the vertices of a region on the device; removeSelected,
// hideSelected and transformSelected then act on them without a host array of flags.
// selectVoxelGrid (section 6g) names one vertex per cell of a regular grid; thin removes all the others.
// selectNeighbours (section 6h) names the vertices with enough others within a radius; removeOutliers removes the rest.
// selectStatistical (section 6n, rtr_statistics.h) names the vertices whose mean distance to their k nearest neighbours is
// ordinary for the cloud; removeStatisticalOutliers removes the rest.
// estimateNormals (section 6o, rtr_normals.h) gives every vertex a unit normal and a curvature from its k nearest
// neighbours; it selects nothing and changes nothing.
// selectClusters (section 6i) names them by the size of their connected cluster; growSelection, removeSmallClusters.
// selectSegments (section 6q, rtr_segments.h) names them by the size of their smooth surface segment -- neighbours whose
// normals agree --: the faces of a room where selectClusters sees one cluster; removeSmallSegments.
// selectNear (section 6k) names the vertices within a radius of GIVEN points, and the given points near a vertex.
// appendNewPoints appends only the given points with no vertex within a radius: a scan merged without duplicates.
// nearestPoints (section 6l) finds for every given point the nearest vertex within a radius and its squared distance;
// matchPoints also returns the matched vertices' coordinates and colours: one ICP step with a fit and transformPoints.
// registerPoints (section 6p, rtr_register.h) aligns a scan to the vertices: ICP steps whose sums and fit are exact.
// nearestKPoints (section 6m) finds the k nearest vertices within a radius, sorted: the input of normals and density.
// fitPlane (section 6j) finds the plane with the most vertices within a distance of it; selectPlane, segmentPlane.
// extractSelected / extractAll (section 2e) read vertices back out in upload order, as appendPoints takes them.
// writeSelected / writePoints / colorSelected (section 2f) put edited vertices and colours back where they came from:
// indices, the keep mask and the selection stay.
//
// computeFull (project_cloud.h:17-18, project_cloud.cu:437-493) needs libtorch: define RTR_WITH_TORCH
// before including this header (and link libtorch); without it the class has the two projection
// methods and tensor(), the device pointer computeFull hands to the U-Net.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#ifdef RTR_WITH_TORCH
#include <torch/script.h>

#include <cstring>
#include <filesystem>
#endif

#include "rtr_normals.h"
#include "rtr_register.h"
#include "rtr_segments.h"
#include "rtr_statistics.h"

namespace rtr {

class ProjectCloud {
public:
    template <class Grid>
    explicit ProjectCloud(const Grid& grid, const std::string& modelFilename = std::string(""), int device = 0,
                          bool point_ids = false)
        : model_filename_(modelFilename) {
        // OctreeGrid::getVertexPositions / getVertexColors (Octreegrid.h:162-180)
        std::vector<float> xyzw;
        std::vector<uint8_t> rgba;
        for (const auto& pair : grid) {
            for (const auto& p : pair.second.positions) {
                xyzw.push_back(p.x); xyzw.push_back(p.y); xyzw.push_back(p.z); xyzw.push_back(1.0f);
            }
            for (const auto& c : pair.second.colors) {
                rgba.push_back(c[0]); rgba.push_back(c[1]); rgba.push_back(c[2]); rgba.push_back(255);
            }
        }
        if (rtr_abi_version() != RTR_ABI_VERSION)  // (a library built from another rtr.h: struct sizes may differ)
            throw std::runtime_error("librtr_hip.so has ABI version " + std::to_string(rtr_abi_version()) +
                                     ", this header is version " + std::to_string(RTR_ABI_VERSION));
        check(nullptr, rtr_create(&ctx_, device));
        if (point_ids) check(ctx_, rtr_set_option(ctx_, "point_ids", 1));
        // (the library's default upload policy: the point order is measured and the cloud Morton-sorted once when its
        // 256-point chunks are not compact -- the grid's 0.25 m blocks are unordered inside -- then packed losslessly)
        check(ctx_, rtr_upload_points(ctx_, xyzw.data(), 16, rgba.data(), 4, xyzw.size() / 4));
#ifdef RTR_WITH_TORCH
        load_model(device);
#endif
    }
    // Appends a grid, flattened like the constructor (rtr.h section 2b)
    template <class Grid>
    void appendPoints(const Grid& grid) {
        std::vector<float> xyzw;
        std::vector<uint8_t> rgba;
        for (const auto& pair : grid) {
            for (const auto& p : pair.second.positions) {
                xyzw.push_back(p.x); xyzw.push_back(p.y); xyzw.push_back(p.z); xyzw.push_back(1.0f);
            }
            for (const auto& c : pair.second.colors) {
                rgba.push_back(c[0]); rgba.push_back(c[1]); rgba.push_back(c[2]); rgba.push_back(255);
            }
        }
        appendPoints(xyzw.data(), 16, rgba.data(), 4, xyzw.size() / 4);
    }
    // Appends m points from host memory, strides as in rtr_upload_points (16 / 4: float4 / uchar4, 12 / 3: tight)
    void appendPoints(const float* xyz, size_t xyz_stride_bytes, const uint8_t* rgb, size_t rgb_stride_bytes, size_t m) {
        check(ctx_, rtr_append_points(ctx_, xyz, xyz_stride_bytes, rgb, rgb_stride_bytes, m));
    }
    ProjectCloud(const ProjectCloud&) = delete;  // owns device buffers (the reference forgets this)
    ProjectCloud& operator=(const ProjectCloud&) = delete;
    ~ProjectCloud() { rtr_destroy(ctx_); }

    template <class Calibration, class Extrinsics, class Image>
    int computeRGBD(const Calibration& calibration, const Extrinsics& extrinsics, Image* color, Image* depth) {
        return frame(calibration, extrinsics, color, depth, false);
    }
    template <class Calibration, class Extrinsics, class Image>
    int computeFilteredRGBD(const Calibration& calibration, const Extrinsics& extrinsics, Image* color, Image* depth) {
        return frame(calibration, extrinsics, color, depth, true);
    }
    // Several views in one pass over the cloud (rtr.h section 6c): extrinsics[v] -> colors[v] / depths[v] (either entry
    // may be null; both vectors as long as `extrinsics`, at most RTR_MAX_VIEWS), what computeRGBD /
    // computeFilteredRGBD would write for that pose.  Returns 1, or -1 when every output is null.
    template <class Calibration, class Extrinsics, class Image>
    int computeRGBDViews(const Calibration& calibration, const std::vector<Extrinsics>& extrinsics,
                         const std::vector<Image*>& colors, const std::vector<Image*>& depths) {
        return views(calibration, extrinsics, colors, depths, false);
    }
    template <class Calibration, class Extrinsics, class Image>
    int computeFilteredRGBDViews(const Calibration& calibration, const std::vector<Extrinsics>& extrinsics,
                                 const std::vector<Image*>& colors, const std::vector<Image*>& depths) {
        return views(calibration, extrinsics, colors, depths, true);
    }
    // literal nullptr for one output, as in cloudreader.cpp:246 `computeRGBD(calib, pose, nullptr, &depth)`
    template <class Calibration, class Extrinsics, class Image>
    int computeRGBD(const Calibration& c, const Extrinsics& e, std::nullptr_t, Image* depth) {
        return frame(c, e, static_cast<Image*>(nullptr), depth, false);
    }
    template <class Calibration, class Extrinsics, class Image>
    int computeRGBD(const Calibration& c, const Extrinsics& e, Image* color, std::nullptr_t) {
        return frame(c, e, color, static_cast<Image*>(nullptr), false);
    }
    template <class Calibration, class Extrinsics>
    int computeRGBD(const Calibration&, const Extrinsics&, std::nullptr_t, std::nullptr_t) { return -1; }
    template <class Calibration, class Extrinsics, class Image>
    int computeFilteredRGBD(const Calibration& c, const Extrinsics& e, std::nullptr_t, Image* depth) {
        return frame(c, e, static_cast<Image*>(nullptr), depth, true);
    }
    template <class Calibration, class Extrinsics, class Image>
    int computeFilteredRGBD(const Calibration& c, const Extrinsics& e, Image* color, std::nullptr_t) {
        return frame(c, e, color, static_cast<Image*>(nullptr), true);
    }
    template <class Calibration, class Extrinsics>
    int computeFilteredRGBD(const Calibration&, const Extrinsics&, std::nullptr_t, std::nullptr_t) { return -1; }
#ifdef RTR_WITH_TORCH
    // computeFull (project_cloud.cu:437-493): projection + prefilter, then the TorchScript model on the
    // RESIDENT fp16 {1,5,H,W} tensor (torch::from_blob, no copy: :471), output[0] permuted to H x W x 3
    // (:475) and converted like cv::Mat::convertTo(CV_8UC3, 255.0) (:480: scale, round half to even,
    // saturate); depth <- the prefiltered depth buffer (:485).  Either output may be null; returns 1.
    // The projector runs on HIP's default stream here, which is torch's current stream unless the caller
    // changed it.  One host synchronisation sits between the frame and the model: a frame that overflowed the
    // adaptive extent pool is rendered again there, so the model never reads a tensor with dropped entries.
    template <class Calibration, class Extrinsics, class Image>
    int computeFull(const Calibration& calibration, const Extrinsics& extrinsics, Image* color, Image* depth) {
        if (!has_model_) throw std::runtime_error("rtr: No model file name given, computeFull will not work");  // :247
        const int W = calibration.getWidth(), H = calibration.getHeight();
        float P[16];
        projection(calibration, extrinsics, P);
        check(ctx_, rtr_set_resolution(ctx_, W, H));
        check(ctx_, rtr_render(ctx_, P, 1));
        // (a frame that overflowed the adaptive extent pool is rendered again here, before the model reads it)
        check(ctx_, rtr_synchronize(ctx_));
        torch::Tensor input = torch::from_blob(tensor(), {1, 5, H, W},
                                               torch::TensorOptions().dtype(torch::kFloat16).device(torch::kCUDA, device_));
        torch::NoGradGuard no_grad;
        torch::Tensor output = model_.forward({input}).toTensor();
        output = output[0].permute({1, 2, 0}).contiguous();
        if (color != nullptr) {
            torch::Tensor u8 = output.to(torch::kFloat32).mul(255.0).round().clamp(0.0, 255.0).to(torch::kUInt8).cpu();
            std::memcpy(color->template ptr<uint8_t>(), u8.data_ptr<uint8_t>(), (size_t)W * H * 3);
        }
        if (depth != nullptr)
            check(ctx_, rtr_download_buffer(ctx_, RTR_BUF_DEPTH, depth->template ptr<float>(), (size_t)W * H * 4));
        return 1;
    }
    template <class Calibration, class Extrinsics, class Image>
    int computeFull(const Calibration& c, const Extrinsics& e, Image* color, std::nullptr_t) {
        return computeFull(c, e, color, static_cast<Image*>(nullptr));
    }
    template <class Calibration, class Extrinsics, class Image>
    int computeFull(const Calibration& c, const Extrinsics& e, std::nullptr_t, Image* depth) {
        return computeFull(c, e, static_cast<Image*>(nullptr), depth);
    }
    // a model object instead of a file under $HOME/.render_cache (tests, callers that build their own)
    void set_model(torch::jit::Module m) {
        model_ = std::move(m);
        model_.to(torch::Device(torch::kCUDA, device_));
        has_model_ = true;
        check(ctx_, rtr_set_stream(ctx_, nullptr));
    }
#endif
    // computeFull (project_cloud.cu:437-493) = computeFilteredRGBD + the caller's U-Net on this
    // device pointer: torch::from_blob(tensor(), {1,5,H,W}, fp16, kCUDA)   (project_cloud.cu:471)
    void* tensor() const {
        void* p = nullptr;
        check(ctx_, rtr_device_buffer(ctx_, RTR_BUF_TENSOR, &p, nullptr));
        return p;
    }
    rtr_ctx* context() const { return ctx_; }

    // Clip planes (rtr.h section 6d): every later frame leaves out the points outside any of `count` (<= 8) world-space
    // half-spaces {a, b, c, d} (planes: count x 4 floats) -- kept iff ((a x + b y) + c z) + d >= 0 in fp32 for each.
    void setClipPlanes(const float* planes, int count) { check(ctx_, rtr_set_clip_planes(ctx_, count, planes)); }
    // Keeps only the points inside the box lo <= q <= hi, q = M p (M: 4x4 row-major world -> box; null: the world axes,
    // where the test is exactly lo <= p <= hi per axis, faces included).  With M the six planes are computed in double
    // and rounded to float once; those float planes define what is kept.
    void setClipBox(const float lo[3], const float hi[3], const double* M = nullptr) {
        float pl[6][4] = {};
        for (int k = 0; k < 3; ++k) {
            if (!M) {
                pl[2 * k][k] = 1.f, pl[2 * k][3] = -lo[k];
                pl[2 * k + 1][k] = -1.f, pl[2 * k + 1][3] = hi[k];
                continue;
            }
            for (int j = 0; j < 3; ++j) {
                pl[2 * k][j] = (float)M[4 * k + j];
                pl[2 * k + 1][j] = (float)-M[4 * k + j];
            }
            pl[2 * k][3] = (float)(M[4 * k + 3] - (double)lo[k]);
            pl[2 * k + 1][3] = (float)((double)hi[k] - M[4 * k + 3]);
        }
        setClipPlanes(&pl[0][0], 6);
    }
    void clearClip() { check(ctx_, rtr_set_clip_planes(ctx_, 0, nullptr)); }

    // Keep mask (rtr.h section 6e): every later frame leaves out the vertices whose flag is 0 (keep: one flag per vertex,
    // in the order the constructor uploads -- the indices of computePointIds / visible_points).
    void setPointKeep(const std::vector<uint8_t>& keep) {
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        if (keep.size() != n) throw std::invalid_argument("setPointKeep: one flag per vertex");
        std::vector<uint32_t> words((size_t)((n + 31) / 32), 0u);
        for (size_t i = 0; i < keep.size(); ++i)
            if (keep[i]) words[i / 32] |= 1u << (i % 32);
        check(ctx_, rtr_set_point_keep(ctx_, words.data(), words.size()));
    }
    // Hides the vertices `indices` as well, on top of the mask in force (none: every vertex kept).
    void hidePoints(const std::vector<uint64_t>& indices) {
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        std::vector<uint32_t> words((size_t)((n + 31) / 32), 0xFFFFFFFFu);
        int set = 0;
        check(ctx_, rtr_get_option(ctx_, "point_keep", &set));
        if (set) check(ctx_, rtr_download_buffer(ctx_, RTR_BUF_POINT_KEEP, words.data(), words.size() * 4));
        for (uint64_t i : indices) {
            if (i >= n) throw std::out_of_range("hidePoints: index past the vertex count");
            words[(size_t)(i / 32)] &= ~(1u << (i % 32));
        }
        check(ctx_, rtr_set_point_keep(ctx_, words.data(), words.size()));
    }
    void clearPointKeep() { check(ctx_, rtr_set_point_keep(ctx_, nullptr, 0)); }
    // Removal (rtr.h section 2c): takes the vertices `indices` out of the resident cloud for good, giving their memory
    // back; the others keep their order and are renumbered 0 .. n' - 1 (the indices of computePointIds, visible_points,
    // hidePoints and later appends).
    void removePoints(const std::vector<uint64_t>& indices) {
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        std::vector<uint32_t> words((size_t)((n + 31) / 32), 0xFFFFFFFFu);
        for (uint64_t i : indices) {
            if (i >= n) throw std::out_of_range("removePoints: index past the vertex count");
            words[(size_t)(i / 32)] &= ~(1u << (i % 32));
        }
        check(ctx_, rtr_remove_points(ctx_, words.data(), words.size()));
    }
    // Moving (rtr.h section 2d): the vertices [first, first + count) (default: to the last one) move by M, row-major 4 x 4
    // whose bottom row must be exactly 0 0 0 1 (std::invalid_argument otherwise); its other twelve elements are rounded
    // to float once.  A range past the vertex count throws std::out_of_range.  The whole cloud moves without a selection
    // (any cloud, sorted or not); a part of a cloud the library may sort needs point_ids = true.
    void transformPoints(const double M[16], uint64_t first = 0, uint64_t count = UINT64_MAX) {
        if (!(M[12] == 0.0 && M[13] == 0.0 && M[14] == 0.0 && M[15] == 1.0))
            throw std::invalid_argument("transformPoints: the bottom row of M must be exactly 0 0 0 1");
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        if (first > n || (count != UINT64_MAX && count > n - first))
            throw std::out_of_range("transformPoints: the range exceeds the vertex count");
        if (count == UINT64_MAX) count = n - first;
        float m[12];
        for (int i = 0; i < 12; ++i) m[i] = (float)M[i];
        if (count == 0) return;
        if (first == 0 && count == n) {
            check(ctx_, rtr_transform_points(ctx_, m, nullptr, 0));
            return;
        }
        std::vector<uint32_t> words((size_t)((n + 31) / 32), 0u);
        for (uint64_t i = first; i < first + count; ++i) words[(size_t)(i / 32)] |= 1u << (i % 32);
        check(ctx_, rtr_transform_points(ctx_, m, words.data(), words.size()));
    }
    // Removes the vertices the keep mask in force hides, then clears the mask (frames unchanged; nothing without a mask).
    void commitPointKeep() {
        int set = 0;
        check(ctx_, rtr_get_option(ctx_, "point_keep", &set));
        if (!set) return;
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        std::vector<uint32_t> words((size_t)((n + 31) / 32), 0u);
        check(ctx_, rtr_download_buffer(ctx_, RTR_BUF_POINT_KEEP, words.data(), words.size() * 4));
        check(ctx_, rtr_remove_points(ctx_, words.data(), words.size()));
        check(ctx_, rtr_set_point_keep(ctx_, nullptr, 0));
    }

    // Selection (rtr.h section 6f): the vertices every half-space of `planes` (count x 4 floats, the contract of
    // setClipPlanes) keeps -- outside: the vertices NOT inside -- combined with the selection so far by op
    // (RTR_SELECT_REPLACE / ADD / SUBTRACT / INTERSECT / TOGGLE).  Returns the number selected afterwards.  point_ids = true
    // when the cloud may be sorted; the clip planes and the keep mask in force play no part.
    uint64_t selectPlanes(const float* planes, int count, int op = RTR_SELECT_REPLACE, bool outside = false) {
        uint64_t st[4] = {0, 0, 0, 0};
        check(ctx_, rtr_select_points(ctx_, count, planes, nullptr, nullptr, op | (outside ? RTR_SELECT_OUTSIDE : 0), st));
        return st[0];
    }
    // selectPlanes of the box lo <= q <= hi, q = M p: the six planes of setClipBox.
    uint64_t selectBox(const float lo[3], const float hi[3], const double* M = nullptr, int op = RTR_SELECT_REPLACE,
                       bool outside = false) {
        float pl[6][4] = {};
        for (int k = 0; k < 3; ++k) {
            if (!M) {
                pl[2 * k][k] = 1.f, pl[2 * k][3] = -lo[k];
                pl[2 * k + 1][k] = -1.f, pl[2 * k + 1][3] = hi[k];
                continue;
            }
            for (int j = 0; j < 3; ++j) {
                pl[2 * k][j] = (float)M[4 * k + j];
                pl[2 * k + 1][j] = (float)-M[4 * k + j];
            }
            pl[2 * k][3] = (float)(M[4 * k + 3] - (double)lo[k]);
            pl[2 * k + 1][3] = (float)((double)hi[k] - M[4 * k + 3]);
        }
        return selectPlanes(&pl[0][0], 6, op, outside);
    }
    // The vertices computeRGBD with this calibration and pose splats onto a pixel x0 <= px < x1, y0 <= py < y1, hidden
    // behind others or not (a rubber band on the screen).
    template <class Calibration, class Extrinsics>
    uint64_t selectRect(const Calibration& calibration, const Extrinsics& extrinsics, int x0, int y0, int x1, int y1,
                        int op = RTR_SELECT_REPLACE) {
        float P[16];
        projection(calibration, extrinsics, P);
        check(ctx_, rtr_set_resolution(ctx_, calibration.getWidth(), calibration.getHeight()));
        const int rect[4] = {x0, y0, x1, y1};
        uint64_t st[4] = {0, 0, 0, 0};
        check(ctx_, rtr_select_points(ctx_, 0, nullptr, P, rect, op, st));
        return st[0];
    }
    // One vertex per cell of a regular grid (section 6g): of the vertices that fall into one cell of size cell[0..2],
    // counted from origin (nullptr: 0 0 0), the one with the smallest vertex index is selected where the cell holds at
    // least min_count vertices; outside: every vertex but those.  Combined with the selection so far by op.  Returns
    // the number selected afterwards.  point_ids = true when the cloud may be sorted.
    uint64_t selectVoxelGrid(const float cell[3], const float origin[3] = nullptr, uint32_t min_count = 1,
                             int op = RTR_SELECT_REPLACE, bool outside = false) {
        const float zero[3] = {0.f, 0.f, 0.f};
        uint64_t st[4];
        check(ctx_, rtr_select_voxel_grid(ctx_, origin ? origin : zero, cell, min_count, op | (outside ? RTR_SELECT_OUTSIDE : 0), st));
        return st[0];
    }
    // Thins the resident cloud to one vertex per cubic cell of size `cell` for good: every vertex but the cells'
    // representatives is selected and removed.  Returns the number of vertices left.
    uint64_t thin(float cell) {
        const float c3[3] = {cell, cell, cell};
        selectVoxelGrid(c3, nullptr, 1, RTR_SELECT_REPLACE, true);
        removeSelected();
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        return n;
    }
    // The vertices with at least min_neighbours other vertices within `radius` (section 6h, the radius outlier filter;
    // the distance test is exact fp32, inclusive, and a vertex is never its own neighbour); outside: every vertex but
    // those -- the outliers, non-finite vertices included.  Combined with the selection so far by op.  Returns the
    // number selected afterwards.  point_ids = true when the cloud may be sorted.
    uint64_t selectNeighbours(float radius, uint32_t min_neighbours, int op = RTR_SELECT_REPLACE, bool outside = false) {
        uint64_t st[4];
        check(ctx_, rtr_select_neighbours(ctx_, radius, min_neighbours, op | (outside ? RTR_SELECT_OUTSIDE : 0), st));
        return st[0];
    }
    // Takes the vertices with fewer than min_neighbours others within `radius` out of the resident cloud for good: they
    // are selected (replacing the selection) and removed.  Returns the number removed.
    uint64_t removeOutliers(float radius, uint32_t min_neighbours) {
        const uint64_t gone = selectNeighbours(radius, min_neighbours, RTR_SELECT_REPLACE, true);
        removeSelected();
        return gone;
    }
    // The vertices whose mean distance to their k (1 .. RTR_STAT_MAX_K) nearest neighbours within `radius` is at most
    // mu + std_mul * sigma, the moments of that mean distance over the cloud (section 6n, the statistical outlier filter:
    // exact fp32 per vertex, fp64 moments in a fixed order); outside: every vertex but those -- the outliers, isolated and
    // non-finite vertices included.  Combined with the selection so far by op.  mean_dist / found (nullptr: none; host or
    // device memory, one entry per vertex): the mean distances and min(k, neighbours); moments (nullptr: none): mu,
    // sigma and the threshold used.  Returns the number selected afterwards.  point_ids = true when the cloud may be sorted.
    uint64_t selectStatistical(uint32_t k, float radius, double std_mul = 1.0, int op = RTR_SELECT_REPLACE, bool outside = false,
                               float* mean_dist = nullptr, uint32_t* found = nullptr, double* moments = nullptr) {
        uint64_t st[4];
        check(ctx_, rtr_select_statistical(ctx_, k, radius, std_mul, 0, op | (outside ? RTR_SELECT_OUTSIDE : 0), mean_dist, found, moments, st));
        return st[0];
    }
    // Takes the statistical outliers out of the resident cloud for good: they are selected (replacing the selection) and
    // removed.  Returns the number removed.
    uint64_t removeStatisticalOutliers(uint32_t k, float radius, double std_mul = 1.0) {
        const uint64_t gone = selectStatistical(k, radius, std_mul, RTR_SELECT_REPLACE, true);
        removeSelected();
        return gone;
    }
    // The unit normal and the curvature of every vertex, from a PCA over the vertex and its k (1 .. RTR_NORMAL_MAX_K)
    // nearest neighbours within `radius` (section 6o: exact, reproducible bit for bit, independent of the resident order).
    // normals: 3 floats per vertex; curvature (nullptr: none): the surface variation, one float per vertex; found (nullptr:
    // none): min(k, neighbours) per vertex -- each in host or device memory, in the order of the vertices.  A vertex with
    // fewer than RTR_NORMAL_MIN_FOUND neighbours gets (0, 0, 0) and +inf.  viewpoint (nullptr: none): three floats towards
    // which every normal is turned.  Nothing is selected or changed.  Returns the number of vertices with a normal.
    // point_ids = true when the cloud may be sorted.
    uint64_t estimateNormals(uint32_t k, float radius, float* normals, float* curvature = nullptr, uint32_t* found = nullptr,
                             const float* viewpoint = nullptr) {
        uint64_t st[4];
        check(ctx_, rtr_estimate_normals(ctx_, k, radius, viewpoint ? RTR_NORMAL_VIEWPOINT : 0, viewpoint, normals, curvature, found, st));
        return st[0];
    }
    // The vertices whose connected cluster within `radius` (section 6i, Euclidean clustering over section 6h's exact
    // relation) holds at least min_points and, unless max_points is 0, at most max_points vertices; seeded: only the
    // clusters that hold a vertex selected before the call; outside: every vertex but those.  Combined with the
    // selection so far by op.  labels (nullptr: none; host or device memory, one uint32_t per vertex): the label of every
    // vertex's cluster, the smallest vertex index among its members.  Returns the number selected afterwards.
    // point_ids = true when the cloud may be sorted.
    uint64_t selectClusters(float radius, uint32_t min_points = 1, uint32_t max_points = 0, bool seeded = false,
                            int op = RTR_SELECT_REPLACE, bool outside = false, uint32_t* labels = nullptr) {
        uint64_t st[4];
        check(ctx_, rtr_select_clusters(ctx_, radius, min_points, max_points, seeded ? RTR_CLUSTER_SEEDED : 0,
                                        op | (outside ? RTR_SELECT_OUTSIDE : 0), labels, st));
        return st[0];
    }
    // Grows the selection to every vertex connected to it by steps of at most `radius`.  Returns the number selected.
    uint64_t growSelection(float radius) { return selectClusters(radius, 1, 0, true); }
    // Distance to given points (rtr.h section 6k): selects the vertices that have one of the m given points (host memory,
    // strides as appendPoints takes them) within `radius` (outside: every vertex but those).  near_words: resized to
    // (m + 31) / 32 words, bit j set = given point j has a vertex within radius.  Returns the number selected afterwards.
    uint64_t selectNear(const float* xyz, size_t xyz_stride_bytes, size_t m, float radius, int op = RTR_SELECT_REPLACE,
                        bool outside = false, std::vector<uint32_t>* near_words = nullptr) {
        uint64_t st[4];
        if (near_words) near_words->assign((m + 31) / 32, 0u);
        check(ctx_, rtr_select_near(ctx_, xyz, xyz_stride_bytes, m, radius, 0, op | (outside ? RTR_SELECT_OUTSIDE : 0),
                                    near_words ? near_words->data() : nullptr, st));
        return st[0];
    }
    // Appends of the m given points exactly those with no vertex within `radius`, in their order (the search leaves
    // the selection as it is; appending even one point drops it, as appendPoints does).  A scan is not thinned against itself: thin it first, or the cloud afterwards (selectVoxelGrid, thin).
    // Returns the number appended.
    size_t appendNewPoints(const float* xyz, size_t xyz_stride_bytes, const uint8_t* rgb, size_t rgb_stride_bytes, size_t m,
                           float radius) {
        std::vector<uint32_t> near((m + 31) / 32 + 1, 0u);
        check(ctx_, rtr_select_near(ctx_, xyz, xyz_stride_bytes, m, radius, RTR_NEAR_GIVEN_ONLY, 0, near.data(), nullptr));
        std::vector<float> v;
        std::vector<uint8_t> c;
        for (size_t j = 0; j < m; ++j) {
            if ((near[j / 32] >> (j % 32)) & 1u) continue;
            const float* p = reinterpret_cast<const float*>(reinterpret_cast<const uint8_t*>(xyz) + j * xyz_stride_bytes);
            const uint8_t* q = rgb + j * rgb_stride_bytes;
            v.insert(v.end(), p, p + 3);
            c.insert(c.end(), q, q + 3);
        }
        if (!c.empty()) appendPoints(v.data(), 12, c.data(), 3, c.size() / 3);
        return c.size() / 3;
    }
    // The nearest vertex to each given point (rtr.h section 6l): for every one of the m given points (host memory, strides
    // as appendPoints takes them) the upload index of the vertex closest to it within `radius` -- of equal distances the
    // smallest index -- and its squared distance, float32 bit for bit; RTR_NEAREST_NONE and +inf where there is none.
    struct Nearest {
        std::vector<uint32_t> index;  // m: upload index, or RTR_NEAREST_NONE
        std::vector<float> dist2;     // m: squared distance, or +inf
    };
    Nearest nearestPoints(const float* xyz, size_t xyz_stride_bytes, size_t m, float radius) {
        Nearest r;
        r.index.assign(m, RTR_NEAREST_NONE);
        r.dist2.assign(m, 0.f);
        check(ctx_, rtr_nearest_points(ctx_, xyz, xyz_stride_bytes, m, radius, 0, r.index.data(), r.dist2.data(), nullptr, nullptr, nullptr));
        return r;
    }
    // The k nearest vertices to each given point (rtr.h section 6m): row j of index / dist2 (k entries at [j * k]) holds the
    // vertices within `radius` of given point j in ascending order of (squared distance bits, upload index), the first
    // min(k, candidates) of them, RTR_NEAREST_NONE and +inf behind them; found[j] is the number of real entries.
    // 1 <= k <= RTR_NEAREST_MAX_K.  For the neighbours of the vertices themselves ask for k + 1 and drop the entry whose
    // index is the vertex's own.
    struct NearestK {
        std::vector<uint32_t> index;  // m * k: upload index, or RTR_NEAREST_NONE
        std::vector<float> dist2;     // m * k: squared distance, or +inf
        std::vector<uint32_t> found;  // m: real entries of the row
        uint32_t k;
    };
    NearestK nearestKPoints(const float* xyz, size_t xyz_stride_bytes, size_t m, uint32_t k, float radius) {
        NearestK r;
        r.k = k;
        r.index.assign(m * (size_t)k, RTR_NEAREST_NONE);
        r.dist2.assign(m * (size_t)k, 0.f);
        r.found.assign(m, 0u);
        check(ctx_, rtr_nearest_k_points(ctx_, xyz, xyz_stride_bytes, m, radius, k, 0, r.index.data(), r.dist2.data(), r.found.data(), nullptr));
        return r;
    }
    // nearestPoints with the matched vertices themselves: vertices / colors hold 3 values per given point, the resident
    // coordinates and colours of its winner bit for bit, zero where there is no match.  One extract of the distinct
    // winners.  With a rigid fit of the matched given points onto `vertices` and transformPoints: one ICP step.
    struct Match {
        std::vector<uint32_t> index;
        std::vector<float> dist2;
        std::vector<float> vertices;  // 3 m
        std::vector<uint8_t> colors;  // 3 m
    };
    Match matchPoints(const float* xyz, size_t xyz_stride_bytes, size_t m, float radius) {
        Nearest nn = nearestPoints(xyz, xyz_stride_bytes, m, radius);
        Match r;
        r.vertices.assign(3 * m, 0.f);
        r.colors.assign(3 * m, (uint8_t)0);
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        std::vector<uint32_t> words((size_t)((n + 31) / 32), 0u), idx;
        bool any = false;
        for (size_t j = 0; j < m; ++j) {
            const uint32_t u = nn.index[j];
            if (u == RTR_NEAREST_NONE) continue;
            words[u / 32] |= 1u << (u % 32);
            any = true;
        }
        if (any) {
            std::vector<float> v;
            std::vector<uint8_t> c;
            extract(words.data(), words.size(), v, c, &idx);  // (ascending upload index: the distinct winners, sorted)
            for (size_t j = 0; j < m; ++j) {
                if (nn.index[j] == RTR_NEAREST_NONE) continue;
                const size_t at = (size_t)(std::lower_bound(idx.begin(), idx.end(), nn.index[j]) - idx.begin());
                std::memcpy(&r.vertices[3 * j], &v[3 * at], 12);
                std::memcpy(&r.colors[3 * j], &c[3 * at], 3);
            }
        }
        r.index = std::move(nn.index);
        r.dist2 = std::move(nn.dist2);
        return r;
    }
    // -- registering a scan (rtr_register.h section 6p) --
    struct Registration {
        double pose[16];          // 4x4 row-major: moves the scan onto the cloud
        std::vector<double> rms;  // the rms residual of every call
        uint64_t stats[4];        // the last call's: pairs used, finite points without one, non-finite points, degenerate
    };
    // step o pose (both 3x4 row-major) in the fixed order of section 6p, part 4
    static void composePose(const double step[12], const double pose[12], double out[12]) {
        double r[12];
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 4; ++b) {
                double v = (step[4 * a] * pose[b] + step[4 * a + 1] * pose[4 + b]) + step[4 * a + 2] * pose[8 + b];
                if (b == 3) v = v + step[4 * a + 3];
                r[4 * a + b] = v;
            }
        std::memcpy(out, r, sizeof r);
    }
    // Aligns the scan (m records of three floats, host or device memory, never written) to the resident cloud by up to
    // `iterations` calls of rtr_register_points, each step composed onto the pose.  point_to_plane with normals nullptr:
    // estimateNormals(16, radius) once, into HOST memory: this header has no device allocator (it does not depend on HIP),
    // so the normals are then uploaded by every call, 12 B per vertex.  For a large cloud call estimateNormals into a
    // device array of your own and pass it here: nothing per-vertex then moves between iterations.
    // Stops at a degenerate step, and at the first call whose pair count equals the previous one's while its rms residual
    // did not fall (that step is not applied).  pose: the 3x4 row-major start, nullptr: the identity.
    Registration registerPoints(const float* xyz, size_t xyz_stride_bytes, size_t m, float radius, int iterations = 20,
                                bool point_to_plane = false, const float* normals = nullptr, const double* pose = nullptr) {
        Registration r{};
        double cur[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        if (pose) std::memcpy(cur, pose, sizeof cur);
        std::vector<float> own;
        if (point_to_plane && !normals) {
            uint64_t n = 0;
            check(ctx_, rtr_num_points(ctx_, &n));
            own.resize((size_t)n * 3);
            estimateNormals(16, radius, own.data());
            normals = own.data();
        }
        bool have_prev = false;
        uint64_t prev_pairs = 0;
        double prev_rms = 0.0;
        for (int it = 0; it < iterations; ++it) {
            double mom[RTR_REGISTER_MOMENTS], step[12];
            check(ctx_, rtr_register_points(ctx_, xyz, xyz_stride_bytes, m, radius, point_to_plane ? RTR_REGISTER_POINT_TO_PLANE : 0, cur,
                                            point_to_plane ? normals : nullptr, mom, step, r.stats));
            // (an IEEE square root and division: the facades and tests/register_ref.py agree on the bits)
            const double rms = mom[0] > 0.0 ? std::sqrt(mom[point_to_plane ? RTR_REGISTER_MOMENTS - 1 : 16] / mom[0]) : HUGE_VAL;
            r.rms.push_back(rms);
            if (r.stats[3]) break;
            if (have_prev && r.stats[0] == prev_pairs && !(rms < prev_rms)) break;
            have_prev = true, prev_pairs = r.stats[0], prev_rms = rms;
            composePose(step, cur, cur);
        }
        std::memcpy(r.pose, cur, sizeof cur);
        r.pose[12] = r.pose[13] = r.pose[14] = 0.0, r.pose[15] = 1.0;
        return r;
    }
    // Takes the clusters of fewer than min_points vertices within `radius` out of the resident cloud for good: their
    // vertices are selected (replacing the selection) and removed.  Returns the number removed.
    uint64_t removeSmallClusters(float radius, uint32_t min_points) {
        const uint64_t gone = selectClusters(radius, min_points, 0, false, RTR_SELECT_REPLACE, true);
        removeSelected();
        return gone;
    }
    // -- smooth segments (section 6q, rtr_segments.h) --
    // The vertices whose smooth surface segment holds at least min_points and, unless max_points is 0, at most max_points
    // vertices: estimateNormals(k, radius), then rtr_select_segments at the same radius -- neighbours whose normals lie
    // within `angle` (radians, up to sign) and whose curvatures are both <= max_curvature (INFINITY: no limit) are joined,
    // and the segments are the connected components.  cos_angle is the host's std::cos(angle) rounded to float: this one
    // value comes from libm, everything behind it is exact.  The normals and the curvature go through HOST vectors: this
    // header has no device allocator (it does not depend on HIP), so 16 B per vertex come down and go up again.  For a
    // large cloud call estimateNormals into device arrays of your own and rtr_select_segments on them.  seeded, op,
    // outside, labels: as selectClusters.  Returns the number selected afterwards.  point_ids = true when the cloud may
    // be sorted.
    uint64_t selectSegments(float radius, uint32_t k, float angle, float max_curvature, uint32_t min_points = 1, uint32_t max_points = 0,
                            bool seeded = false, int op = RTR_SELECT_REPLACE, bool outside = false, uint32_t* labels = nullptr) {
        uint64_t n = 0, st[4];
        check(ctx_, rtr_num_points(ctx_, &n));
        std::vector<float> normals((size_t)n * 3), curvature((size_t)n);
        estimateNormals(k, radius, normals.data(), curvature.data());
        check(ctx_, rtr_select_segments(ctx_, radius, (float)std::cos((double)angle), normals.data(), curvature.data(), max_curvature, min_points,
                                        max_points, seeded ? RTR_SEGMENT_SEEDED : 0, op | (outside ? RTR_SELECT_OUTSIDE : 0), labels, st));
        return st[0];
    }
    // Takes the smooth segments of fewer than min_points vertices out of the resident cloud for good: their vertices are
    // selected (replacing the selection) and removed.  Returns the number removed.
    uint64_t removeSmallSegments(float radius, uint32_t k, float angle, float max_curvature, uint32_t min_points) {
        const uint64_t gone = selectSegments(radius, k, angle, max_curvature, min_points, 0, false, RTR_SELECT_REPLACE, true);
        removeSelected();
        return gone;
    }
    // -- the dominant plane (rtr.h section 6j) --
    struct Plane {
        float abcd[4];     // unit normal with (c, b, a) lexicographically positive, and the offset
        uint64_t inliers;  // the vertices of the population within dist of it
    };
    // Counts, for each of `count` bands {a, b, c, d_lo, d_hi}, the vertices with u + d_lo >= 0 and -u + d_hi >= 0,
    // u = (a x + b y) + c z in fp32; selected: among the selected vertices only.  The selection stays as it is.
    std::vector<uint64_t> countInBands(const float* bands, uint32_t count, bool selected = false, uint64_t stats[4] = nullptr) {
        std::vector<uint64_t> counts(count);
        check(ctx_, rtr_count_in_bands(ctx_, count, bands, selected ? RTR_BANDS_SELECTED : 0, counts.data(), stats));
        return counts;
    }
    // RANSAC fit of the plane with the most vertices within `dist`: `iterations` candidates through three sampled
    // vertices each (seed: the sampler's stream); selected: among the selected vertices only.  The selection stays as
    // it is.  Throws std::runtime_error when every candidate is degenerate (fewer than three vertices, all samples
    // collinear or coincident).  stats: rtr_fit_plane's.
    Plane fitPlane(float dist, uint32_t iterations = 256, uint64_t seed = 0, bool selected = false, uint64_t stats[4] = nullptr) {
        Plane p{};
        uint64_t st[4] = {0, 0, 0, 0};
        check(ctx_, rtr_fit_plane(ctx_, dist, iterations, seed, selected ? RTR_BANDS_SELECTED : 0, p.abcd, st));
        if (stats) std::memcpy(stats, st, sizeof st);
        if (st[1] == 0) throw std::runtime_error("rtr: fitPlane: every candidate was degenerate");
        p.inliers = st[0];
        return p;
    }
    // Selects the vertices within `dist` of `plane` {a, b, c, d}: rtr_select_points with the two planes {a, b, c, d + dist}
    // and {-a, -b, -c, dist - d} of the fit's band (each sum one fp32 operation), so that with REPLACE the count is
    // exactly fitPlane's.  Returns the number selected afterwards.
    uint64_t selectPlane(const float plane[4], float dist, int op = RTR_SELECT_REPLACE, bool outside = false) {
        volatile float lo = plane[3] + dist, hi = dist - plane[3];  // (volatile: rounded to fp32 whatever the build's flags)
        const float two[8] = {plane[0], plane[1], plane[2], lo, -plane[0], -plane[1], -plane[2], hi};
        uint64_t st[4];
        check(ctx_, rtr_select_points(ctx_, 2, two, nullptr, nullptr, op | (outside ? RTR_SELECT_OUTSIDE : 0), st));
        return st[0];
    }
    // Open3D's segment_plane: fitPlane, then selectPlane of it with REPLACE -- the inliers are the selection.  Peeling a
    // second plane off the rest: segmentPlane, rtr_select_points with no plane and RTR_SELECT_TOGGLE, then
    // fitPlane(dist, iterations, seed, true).
    Plane segmentPlane(float dist, uint32_t iterations = 256, uint64_t seed = 0) {
        const Plane p = fitPlane(dist, iterations, seed);
        selectPlane(p.abcd, dist);
        return p;
    }
    uint64_t selectedCount() {
        if (!has_selection()) return 0;
        uint64_t st[4] = {0, 0, 0, 0};  // (adds the complement of every point: nothing)
        check(ctx_, rtr_select_points(ctx_, 0, nullptr, nullptr, nullptr, RTR_SELECT_ADD | RTR_SELECT_OUTSIDE, st));
        return st[0];
    }
    void clearSelection() { check(ctx_, rtr_clear_selection(ctx_)); }
    // Takes the selected vertices out of the resident cloud for good (see removePoints); the selection is gone.
    void removeSelected() {
        with_complement([&](const uint32_t* words, uint64_t nwords) { check(ctx_, rtr_remove_points(ctx_, words, nwords)); });
        clearSelection();  // (also when nothing was selected)
    }
    // The keep mask becomes everything but the selection (a mask in force is replaced); the selection stays.
    void hideSelected() {
        with_complement([&](const uint32_t* words, uint64_t nwords) { check(ctx_, rtr_set_point_keep(ctx_, words, nwords)); });
    }
    // Moves the selected vertices by M (see transformPoints); the selection stays, naming the same vertices.
    void transformSelected(const double M[16]) {
        if (!(M[12] == 0.0 && M[13] == 0.0 && M[14] == 0.0 && M[15] == 1.0))
            throw std::invalid_argument("transformSelected: the bottom row of M must be exactly 0 0 0 1");
        if (!has_selection()) return;
        float m[12];
        for (int i = 0; i < 12; ++i) m[i] = (float)M[i];
        void* p = nullptr;
        size_t bytes = 0;
        check(ctx_, rtr_device_buffer(ctx_, RTR_BUF_SELECTION, &p, &bytes));
        check(ctx_, rtr_transform_points(ctx_, m, static_cast<const uint32_t*>(p), bytes / 4));
    }

    // Reads the selected vertices back out in upload order (section 2e): tight xyz (3 floats per vertex) and tight colour
    // triples -- the layouts appendPoints(xyz, 12, rgb, 3, m) takes, so the result can be handed to another ProjectCloud
    // -- and, when asked for, their vertex indices.  Returns their number (0 and empty vectors without a selection).
    // Only the chunks holding a selected vertex are decoded; the clip planes and the keep mask play no part.
    uint64_t extractSelected(std::vector<float>& vertices, std::vector<uint8_t>& colors,
                             std::vector<uint32_t>* indices = nullptr) {
        vertices.clear(); colors.clear();
        if (indices) indices->clear();
        if (!has_selection()) return 0;
        void* p = nullptr;
        size_t bytes = 0;
        check(ctx_, rtr_device_buffer(ctx_, RTR_BUF_SELECTION, &p, &bytes));
        return extract(static_cast<const uint32_t*>(p), (uint64_t)(bytes / 4), vertices, colors, indices);
    }
    // Every vertex as it is resident now (after appends, removals and moves), in upload order; a cloud sorted without
    // point_ids comes in the sorted order.  Returns the vertex count.
    uint64_t extractAll(std::vector<float>& vertices, std::vector<uint8_t>& colors) {
        vertices.clear(); colors.clear();
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        if (n == 0) return 0;
        return extract(nullptr, 0, vertices, colors, nullptr);
    }

    // Writing back (rtr.h section 2f), the mirror image of extractSelected: the selected vertices, in ascending vertex
    // index, take the tight records of `vertices` (3 floats each) and `colors` (3 bytes each), as extractSelected returned
    // and the caller edited them.  Either vector may be empty: that stream stays as it is resident.  A size that is not 3 k,
    // or two non-empty vectors of different k, throws std::invalid_argument.  Vertex indices, the keep mask and the
    // selection stay.  Returns the number of vertices written (0 without a selection): min(k, selected).
    uint64_t writeSelected(const std::vector<float>& vertices, const std::vector<uint8_t>& colors) {
        const uint64_t k = write_count(vertices, colors, "writeSelected");
        if (!has_selection() || k == 0) return 0;
        void* p = nullptr;
        size_t bytes = 0;
        check(ctx_, rtr_device_buffer(ctx_, RTR_BUF_SELECTION, &p, &bytes));
        return write(static_cast<const uint32_t*>(p), (uint64_t)(bytes / 4), 0, k, vertices, colors);
    }
    // The vertices [first, first + count) take the records, as transformPoints names a range: count defaults to the
    // records given; a range past the vertex count throws std::out_of_range, fewer records than `count` or a size that is
    // not 3 k std::invalid_argument.  A cloud sorted without point_ids is addressed in its sorted order (extractAll's).
    uint64_t writePoints(uint64_t first, uint64_t count, const std::vector<float>& vertices, const std::vector<uint8_t>& colors) {
        const uint64_t k = write_count(vertices, colors, "writePoints");
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        if (count == UINT64_MAX) count = k;
        if (first > n || count > n - first) throw std::out_of_range("writePoints: the range exceeds the vertex count");
        if (count > k) throw std::invalid_argument("writePoints: fewer records than vertices in the range");
        if (count == 0) return 0;
        return write(nullptr, 0, first, count, vertices, colors);  // (every vertex: rank = vertex index)
    }
    // One colour for every selected vertex (a highlight); the selection stays.  Returns the number coloured.
    uint64_t colorSelected(uint8_t c0, uint8_t c1, uint8_t c2) {
        if (!has_selection()) return 0;
        void* p = nullptr;
        size_t bytes = 0;
        check(ctx_, rtr_device_buffer(ctx_, RTR_BUF_SELECTION, &p, &bytes));
        const uint8_t rgb[3] = {c0, c1, c2};
        uint64_t total = 0;
        check(ctx_, rtr_write_points(ctx_, static_cast<const uint32_t*>(p), (uint64_t)(bytes / 4), 0, UINT64_MAX, nullptr, 0, rgb, 0,
                                     &total));
        return total;
    }

    // Renders the frame (computeRGBD / computeFilteredRGBD without host copies) and returns, per pixel (row-major
    // H x W), the vertex index of the point it shows, -1 for none (empty or prefiltered-away pixels).
    template <class Calibration, class Extrinsics>
    std::vector<int64_t> computePointIds(const Calibration& calibration, const Extrinsics& extrinsics, bool filtered = false) {
        point_pass(calibration, extrinsics, filtered, RTR_POINTS_IDS);
        std::vector<uint32_t> ids((size_t)calibration.getWidth() * calibration.getHeight());
        check(ctx_, rtr_download_buffer(ctx_, RTR_BUF_POINT_ID, ids.data(), ids.size() * 4));
        std::vector<int64_t> out(ids.size());
        for (size_t p = 0; p < ids.size(); ++p) out[p] = ids[p] == 0xFFFFFFFFu ? -1 : (int64_t)ids[p];
        return out;
    }
    // Renders the frame and returns one flag per vertex: 1 for the points that contributed to its colour.
    template <class Calibration, class Extrinsics>
    std::vector<uint8_t> visible_points(const Calibration& calibration, const Extrinsics& extrinsics, bool filtered = false) {
        point_pass(calibration, extrinsics, filtered, RTR_POINTS_VISIBLE);
        uint64_t n = 0;
        check(ctx_, rtr_num_points(ctx_, &n));
        std::vector<uint32_t> words((size_t)((n + 31) / 32));
        check(ctx_, rtr_download_buffer(ctx_, RTR_BUF_VISIBLE, words.data(), words.size() * 4));
        std::vector<uint8_t> out((size_t)n);
        for (size_t i = 0; i < out.size(); ++i) out[i] = (uint8_t)((words[i / 32] >> (i % 32)) & 1u);
        return out;
    }

private:
    bool has_selection() const {
        int set = 0;
        check(ctx_, rtr_get_option(ctx_, "selection", &set));
        return set != 0;
    }
    // fn(device words of everything but the selection): inverted on the device (RTR_SELECT_TOGGLE) and back
    template <class Fn>
    void with_complement(Fn fn) {
        if (!has_selection())  // (none yet: an empty one)
            check(ctx_, rtr_select_points(ctx_, 0, nullptr, nullptr, nullptr, RTR_SELECT_SUBTRACT, nullptr));
        check(ctx_, rtr_select_points(ctx_, 0, nullptr, nullptr, nullptr, RTR_SELECT_TOGGLE, nullptr));
        void* p = nullptr;
        size_t bytes = 0;
        check(ctx_, rtr_device_buffer(ctx_, RTR_BUF_SELECTION, &p, &bytes));
        try {
            fn(static_cast<const uint32_t*>(p), (uint64_t)(bytes / 4));
        } catch (...) {
            if (has_selection()) rtr_select_points(ctx_, 0, nullptr, nullptr, nullptr, RTR_SELECT_TOGGLE, nullptr);
            throw;
        }
        if (has_selection())  // (a removal drops it)
            check(ctx_, rtr_select_points(ctx_, 0, nullptr, nullptr, nullptr, RTR_SELECT_TOGGLE, nullptr));
    }
    uint64_t extract(const uint32_t* words, uint64_t nwords, std::vector<float>& vertices, std::vector<uint8_t>& colors,
                     std::vector<uint32_t>* indices) {
        uint64_t k = 0;
        check(ctx_, rtr_extract_points(ctx_, words, nwords, 0, 0, nullptr, 0, nullptr, 0, nullptr, &k));
        vertices.resize((size_t)k * 3);
        colors.resize((size_t)k * 3);
        if (indices) indices->resize((size_t)k);
        if (k)
            check(ctx_, rtr_extract_points(ctx_, words, nwords, 0, k, vertices.data(), 12, colors.data(), 3,
                                           indices ? indices->data() : nullptr, nullptr));
        return k;
    }
    // the records of a write: tight triples, an empty vector = that stream stays; -> their number
    static uint64_t write_count(const std::vector<float>& vertices, const std::vector<uint8_t>& colors, const char* fn) {
        if (vertices.size() % 3 || colors.size() % 3)
            throw std::invalid_argument(std::string(fn) + ": vertices and colors hold 3 values per vertex");
        if (!vertices.empty() && !colors.empty() && vertices.size() != colors.size())
            throw std::invalid_argument(std::string(fn) + ": vertices and colors name different numbers of vertices");
        if (vertices.empty() && colors.empty())
            throw std::invalid_argument(std::string(fn) + ": vertices and colors are both empty, nothing to write");
        return (uint64_t)((vertices.empty() ? colors.size() : vertices.size()) / 3);
    }
    uint64_t write(const uint32_t* words, uint64_t nwords, uint64_t first, uint64_t count, const std::vector<float>& vertices,
                   const std::vector<uint8_t>& colors) {
        uint64_t total = 0;
        check(ctx_, rtr_write_points(ctx_, words, nwords, first, count, vertices.empty() ? nullptr : vertices.data(), 12,
                                     colors.empty() ? nullptr : colors.data(), 3, &total));
        return first < total ? (count < total - first ? count : total - first) : 0;
    }
    template <class Calibration, class Extrinsics>
    static void projection(const Calibration& calibration, const Extrinsics& extrinsics, float P[16]) {
        double K[9], E[16];
        const auto Km = calibration.getIntrinsicsMatrix();
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) K[3 * r + c] = Km(r, c);
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) E[4 * r + c] = extrinsics(r, c);
        rtr_compose_projection(K, E, P);  // project_cloud.cu:318
    }
#ifdef RTR_WITH_TORCH
    void load_model(int device) {  // project_cloud.cu:225-250 (throws where the reference exits)
        device_ = device;
        if (model_filename_.empty()) return;  // "No model file name given, computeFull will not work."
        const char* home = std::getenv("HOME");
        const std::string path = (std::filesystem::path(home ? home : "") / ".render_cache" / model_filename_).string();
        if (!std::filesystem::exists(path))
            throw std::runtime_error("rtr: Model file does not exist: " + path + " (export a TorchScript model for this "
                                     "camera resolution first)");
        set_model(torch::jit::load(path));
    }
    torch::jit::Module model_;
    bool has_model_ = false;
    int device_ = 0;
#endif
    template <class Calibration, class Extrinsics, class Image>
    int frame(const Calibration& calibration, const Extrinsics& extrinsics, Image* color, Image* depth, bool filtered) {
        if (color == nullptr && depth == nullptr) return -1;  // project_cloud.cu:270-273
        float P[16];
        projection(calibration, extrinsics, P);
        check(ctx_, rtr_set_resolution(ctx_, calibration.getWidth(), calibration.getHeight()));  // :275-298
        uint8_t* c8 = color ? color->template ptr<uint8_t>() : nullptr;
        float* d32 = depth ? depth->template ptr<float>() : nullptr;
        check(ctx_, filtered ? rtr_project_filtered(ctx_, P, c8, d32) : rtr_project(ctx_, P, c8, d32));
        return 1;
    }
    template <class Calibration, class Extrinsics, class Image>
    int views(const Calibration& calibration, const std::vector<Extrinsics>& extrinsics, const std::vector<Image*>& colors,
              const std::vector<Image*>& depths, bool filtered) {
        const size_t k = extrinsics.size();
        if (k < 1 || k > RTR_MAX_VIEWS || colors.size() != k || depths.size() != k)
            throw std::invalid_argument("rtr: 1..RTR_MAX_VIEWS extrinsics, one colour and one depth entry (or null) each");
        bool any = false;
        for (size_t v = 0; v < k; ++v) any = any || colors[v] != nullptr || depths[v] != nullptr;
        if (!any) return -1;
        std::vector<float> P(16 * k);
        for (size_t v = 0; v < k; ++v) projection(calibration, extrinsics[v], P.data() + 16 * v);
        const int W = calibration.getWidth(), H = calibration.getHeight();
        check(ctx_, rtr_set_resolution(ctx_, W, H));
        check(ctx_, rtr_render_views(ctx_, (int)k, P.data(), filtered ? 1 : 0));
        const size_t npix = (size_t)W * H;
        std::vector<uint8_t> img(k * npix * 3);
        std::vector<float> depth(k * npix);
        check(ctx_, rtr_download_buffer(ctx_, RTR_BUF_VIEW_DEPTH, depth.data(), depth.size() * 4));
        check(ctx_, rtr_download_buffer(ctx_, RTR_BUF_VIEW_IMAGE, img.data(), img.size()));
        for (size_t v = 0; v < k; ++v) {
            if (colors[v]) std::memcpy(colors[v]->template ptr<uint8_t>(), img.data() + v * npix * 3, npix * 3);
            if (depths[v]) std::memcpy(depths[v]->template ptr<float>(), depth.data() + v * npix, npix * 4);
        }
        return 1;
    }
    template <class Calibration, class Extrinsics>
    void point_pass(const Calibration& calibration, const Extrinsics& extrinsics, bool filtered, int what) {
        float P[16];
        projection(calibration, extrinsics, P);
        check(ctx_, rtr_set_resolution(ctx_, calibration.getWidth(), calibration.getHeight()));
        check(ctx_, rtr_render(ctx_, P, filtered ? 1 : 0));
        check(ctx_, rtr_point_pass(ctx_, P, what));
    }
    static void check(const rtr_ctx* c, int rc) {
        if (rc != RTR_OK) throw std::runtime_error(std::string("rtr: ") + rtr_last_error(c));
    }
    rtr_ctx* ctx_ = nullptr;
    std::string model_filename_;
};

}  // namespace rtr
