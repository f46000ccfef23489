// driver.cpp -- runs the reference's own stage kernels on the host, serially.  TEST INFRASTRUCTURE ONLY.
//
//   ref_host <request file> <result file>
//
// The kernels are the reference's text (image_renderer.cuh, compute_point_clouds.cuh, compute_costs.cuh), copied into
// oracle/_ref/src/ by filter_sources.py without their host launchers and compiled behind shim/ref_shim.h.  This file is
// the launchers' replacement: it walks each kernel's grid in a loop (set blockIdx / threadIdx, call the function) and
// does the library steps the launchers do between kernels with the reference's own functors, citing their lines.
// Built with the oracle's float flags (no FMA contraction); oracle.build_ref() also builds it with
// -fsanitize=address,undefined, and the golden generator runs only that build.
//
// The request and result files are bundle.h's.
#include "cuda_renderer/cuda/image_renderer.cuh"
#include "cuda_renderer/cuda/compute_point_clouds.cuh"
#include "cuda_renderer/cuda/compute_costs.cuh"

#include "bundle.h"

using cuda_renderer::Model;

namespace {

// ---- stage RENDER: image_render (image_renderer.cuh:336-496) ------------------------------------------------
// descending: walk the triangle axis of the grid from its last thread to its first.  On the device the order in which
// the triangles of a pose reach a pixel is the scheduler's; the two extremes show what depends on it.
void run_render(const Bundle& q, Bundle& out, bool descending, const std::string& suffix, std::vector<int32_t>* keep_depth,
                std::vector<uint8_t>* keep_rgb) {
    const size_t width = (size_t)q.geti("width"), height = (size_t)q.geti("height");
    const size_t num_tris = q.count("tris") / 9;
    const int num_images = (int)(q.count("poses") / 16);
    const int num_models = (int)q.count("tris_model_count");
    const float* tris = q.ptr<float>("tris", num_tris * 9);
    const uint8_t* tri_rgb = q.ptr<uint8_t>("tri_rgb", num_tris * 3);
    const float occlusion_threshold = q.getf("occlusion_threshold");

    std::vector<Model::Triangle> device_tris(num_tris);
    for (size_t t = 0; t < num_tris; t++) {
        const float* p = tris + 9 * t;
        device_tris[t].v0 = {p[0], p[1], p[2]};
        device_tris[t].v1 = {p[3], p[4], p[5]};
        device_tris[t].v2 = {p[6], p[7], p[8]};
        device_tris[t].color = {tri_rgb[3 * t + 0], tri_rgb[3 * t + 1], tri_rgb[3 * t + 2]};  // model.cpp:92-94
    }
    std::vector<Model::mat4x4> device_poses(num_images);
    for (int i = 0; i < num_images; i++) device_poses[i].init_from_ptr(q.ptr<float>("poses") + 16 * i);
    Model::mat4x4 proj_mat;
    proj_mat.init_from_ptr(q.ptr<float>("proj", 16));
    const int* device_pose_model_map = q.ptr<int32_t>("pose_model", num_images);
    const int* counts = q.ptr<int32_t>("tris_model_count");
    for (int i = 0; i < num_images; i++)
        if (device_pose_model_map[i] < 0 || device_pose_model_map[i] >= num_models) throw std::runtime_error("pose_model out of range");

    const Model::ROI roi = {0, 0, 0, 0};  // :369
    // :371-380 exclusive / inclusive scans of the triangles per model
    std::vector<int> low(num_models), high(num_models);
    int acc = 0;
    for (int m = 0; m < num_models; m++) {
        low[m] = acc;
        acc += counts[m];
        high[m] = acc;
    }
    // :385-398
    std::vector<int> pose_occluded(num_images, 0), pose_occluded_other(num_images, 0);
    std::vector<float> pose_clutter_points(num_images, 0), pose_total_points(num_images, 0);
    const size_t n = (size_t)num_images * width * height;
    std::vector<int32_t> lock_int(n, 0), depth_int(n, INT_MAX);
    std::vector<uint8_t> red_int(n, 0), green_int(n, 0), blue_int(n, 0);

    const int32_t* source_depth = q.ptr<int32_t>("src_depth", width * height);
    const uint8_t* source_red = q.ptr<uint8_t>("src_red", width * height);
    const uint8_t* source_green = q.ptr<uint8_t>("src_green", width * height);
    const uint8_t* source_blue = q.ptr<uint8_t>("src_blue", width * height);
    const uint8_t* source_mask_label = q.ptr<uint8_t>("src_mask", width * height);
    std::vector<int> pose_segmentation_label;
    if (q.has("pose_label")) pose_segmentation_label.assign(q.ptr<int32_t>("pose_label", num_images), q.ptr<int32_t>("pose_label") + num_images);
    const bool use_segmentation_label = !pose_segmentation_label.empty();  // :426-432
    const int device_single_result_image = 0;

    // :444-463 the launch: grid ((T + 255) / 256, num_images), THREADS_PER_BLOCK threads
    gridDim.x = (unsigned)((num_tris + THREADS_PER_BLOCK - 1) / THREADS_PER_BLOCK);
    gridDim.y = (unsigned)num_images;
    blockDim.x = THREADS_PER_BLOCK;
    blockDim.y = 1;
    threadIdx.y = 0;
    for (unsigned by = 0; by < gridDim.y; by++)
        for (unsigned bi = 0; bi < gridDim.x; bi++)
            for (unsigned ti = 0; ti < blockDim.x; ti++) {
                blockIdx.y = by;
                blockIdx.x = descending ? gridDim.x - 1 - bi : bi;
                threadIdx.x = descending ? blockDim.x - 1 - ti : ti;
                cuda_renderer::image_renderer::render_triangle_multi(
                    device_tris.data(), device_tris.size(), device_poses.data(), (size_t)num_images, depth_int.data(), width,
                    height, device_pose_model_map, low.data(), high.data(), proj_mat, roi, red_int.data(), green_int.data(),
                    blue_int.data(), source_depth, source_red, source_green, source_blue, pose_occluded.data(),
                    device_single_result_image, lock_int.data(), pose_occluded_other.data(), pose_clutter_points.data(),
                    pose_total_points.data(), source_mask_label, data_of(pose_segmentation_label), use_segmentation_label,
                    occlusion_threshold);
            }
    // :465-472 max -> 0 on the depth and on the three colour planes
    const cuda_renderer::image_renderer::max2zero_functor_renderer max2zero;
    for (size_t i = 0; i < n; i++) {
        depth_int[i] = max2zero(depth_int[i]);
        red_int[i] = (uint8_t)max2zero(red_int[i]);
        green_int[i] = (uint8_t)max2zero(green_int[i]);
        blue_int[i] = (uint8_t)max2zero(blue_int[i]);
    }
    for (int v : lock_int)
        if (v != 0) throw std::runtime_error("a pixel lock was left taken");
    const std::vector<int64_t> shape = {num_images, (int64_t)height, (int64_t)width};
    out.put("depth" + suffix, depth_int, shape);
    std::vector<uint8_t> rgb;
    rgb.insert(rgb.end(), red_int.begin(), red_int.end());
    rgb.insert(rgb.end(), green_int.begin(), green_int.end());
    rgb.insert(rgb.end(), blue_int.begin(), blue_int.end());
    out.put("color" + suffix, rgb, {3, num_images, (int64_t)height, (int64_t)width});
    out.put("pose_occluded" + suffix, pose_occluded, {num_images});
    if (keep_depth) *keep_depth = depth_int;
    if (keep_rgb) *keep_rgb = rgb;
}

// ---- stage CLOUD: compute_point_clouds (compute_point_clouds.cuh:188-367) -----------------------------------
// depth: num_poses x H x W; planes: red, green, blue planes of the same shape.  The optional inputs are the launcher's
// optional arguments: label_mask (depth2cloud_global's label_mask_data), bounds + camera_transform (its 3-DoF pair),
// pose_label (the rendered cloud's pose_segmentation_label).
void run_cloud(const Bundle& q, Bundle& out, const int32_t* depth_data, const uint8_t* planes, int num_poses,
               const std::string& prefix) {
    const int width = q.geti("width"), height = q.geti("height"), stride = q.geti("stride");
    const float cx = q.getf("cx"), cy = q.getf("cy"), fx = q.getf("fx"), fy = q.getf("fy"), depth_factor = q.getf("depth_factor");
    const size_t n = (size_t)num_poses * width * height;
    const uint8_t *red_in = planes, *green_in = planes + n, *blue_in = planes + 2 * n;
    const uint8_t* image_label = q.opt<uint8_t>("label_mask", n);
    const double* observed_cloud_bounds = q.opt<double>("bounds", 6);
    const int* pose_segmentation_label_ptr = q.opt<int32_t>("pose_label", num_poses);
    Eigen::Matrix4f transform;
    const Eigen::Matrix4f* camera_transform = nullptr;
    if (q.has("camera_transform")) {
        const float* m = q.ptr<float>("camera_transform", 16);  // row-major in the request
        for (int r = 0; r < 4; r++)
            for (int c = 0; c < 4; c++) transform(r, c) = m[4 * r + c];
        camera_transform = &transform;
    }
    std::vector<int> poses_occluded(num_poses, 0);

    std::vector<int> result_dc_index(n, 0);  // :267
    int* mask_ptr = result_dc_index.data();
    // :270-273 the grid both kernels share
    if (width % stride != 0) throw std::runtime_error("width % stride != 0 (compute_point_clouds.cuh:271 asserts it)");
    blockDim.x = 16;
    blockDim.y = 16;
    gridDim.x = (unsigned)((width / stride * num_poses + blockDim.x - 1) / blockDim.x);
    gridDim.y = (unsigned)((height / stride + blockDim.y - 1) / blockDim.y);
    auto for_each_thread = [&](auto&& kernel) {
        for (unsigned by = 0; by < gridDim.y; by++)
            for (unsigned bx = 0; bx < gridDim.x; bx++)
                for (unsigned ty = 0; ty < blockDim.y; ty++)
                    for (unsigned tx = 0; tx < blockDim.x; tx++) {
                        blockIdx.x = bx;
                        blockIdx.y = by;
                        threadIdx.x = tx;
                        threadIdx.y = ty;
                        kernel();
                    }
    };
    for_each_thread([&] {  // :274-288
        cuda_renderer::image_to_cloud::depth_to_mask(depth_data, mask_ptr, width, height, stride, num_poses, poses_occluded.data(),
                                                     image_label, cx, cy, fx, fy, depth_factor, observed_cloud_bounds,
                                                     camera_transform);
    });
    // :290-292 exclusive scan in place; the count is its last element plus the last mask bit
    const int mask_back_temp = result_dc_index.back();
    int running = 0;
    for (size_t i = 0; i < n; i++) {
        const int m = result_dc_index[i];
        result_dc_index[i] = running;
        running += m;
    }
    const int result_cloud_point_count = result_dc_index.back() + mask_back_temp;
    const size_t P = (size_t)result_cloud_point_count;
    // :295-318 outputs (cudaMallocPitch: rows of at least P floats; a pitch of its own here)
    const size_t cloud_pitch = (P * sizeof(float) + 511) / 512 * 512 + 512;
    std::vector<char> cloud_2d(POINT_DIM * cloud_pitch, 0);
    std::vector<Eigen::Vector3f> cloud_eigen(P, Eigen::Vector3f::Constant(0));
    std::vector<float> cloud_1d(POINT_DIM * P, 0);
    std::vector<uint8_t> cloud_color(POINT_DIM * P, 0);
    std::vector<int> cloud_pose_map(P, 0);
    std::vector<int> cloud_label;
    int* cloud_mask_label = nullptr;
    if (image_label != nullptr || pose_segmentation_label_ptr != nullptr) {
        cloud_label.assign(P, 0);
        cloud_mask_label = data_of(cloud_label);
    }
    for_each_thread([&] {  // :321-346
        cuda_renderer::image_to_cloud::depth_to_2d_cloud(
            depth_data, red_in, green_in, blue_in, reinterpret_cast<float*>(cloud_2d.data()), data_of(cloud_1d),
            data_of(cloud_eigen), cloud_pitch, data_of(cloud_color), result_cloud_point_count, mask_ptr, width, height, cx, cy,
            fx, fy, depth_factor, stride, num_poses, data_of(cloud_pose_map), image_label, cloud_mask_label,
            observed_cloud_bounds, camera_transform, pose_segmentation_label_ptr);
    });
    // the three copies of the cloud the kernel writes must agree
    for (size_t i = 0; i < P; i++)
        for (int d = 0; d < POINT_DIM; d++) {
            const float a = cloud_1d[i + d * P];
            const float b = reinterpret_cast<const float*>(cloud_2d.data() + d * cloud_pitch)[i];
            const float c = cloud_eigen[i](d);
            if (std::memcmp(&a, &b, 4) != 0 || std::memcmp(&a, &c, 4) != 0) throw std::runtime_error("the kernel's cloud copies differ");
        }
    const int32_t count = result_cloud_point_count;
    out.put(prefix + "count", &count, {1});
    out.put(prefix + "xyz", cloud_1d, {POINT_DIM, (int64_t)P});
    out.put(prefix + "color", cloud_color, {POINT_DIM, (int64_t)P});
    out.put(prefix + "pose_map", cloud_pose_map, {(int64_t)P});
    if (image_label != nullptr || pose_segmentation_label_ptr != nullptr)
        out.put(prefix + "label", cloud_label, {(int64_t)P});
    out.put(prefix + "dc_index", result_dc_index, {num_poses, height, width});
}

// ---- stage COST: compute_costs (compute_costs.cuh:293-457) ---------------------------------------------------
void run_costs(const Bundle& q, Bundle& out) {
    const int num_images = q.geti("num_poses"), cost_type = q.geti("cost_type");
    const bool calculate_observed_cost = q.geti("calc_obs_cost") != 0;
    float sensor_resolution = q.getf("sensor_resolution");
    sensor_resolution = sensor_resolution * sensor_resolution;  // renderer.cu:1877
    const float color_distance_threshold = q.getf("color_threshold");
    const int observed_cloud_point_count = q.geti("num_observed");
    const int rendered_cloud_point_count = (int)q.count("knn_dist");
    const size_t O = (size_t)observed_cloud_point_count, P = (size_t)rendered_cloud_point_count;
    const uint8_t* observed_cloud_color = q.ptr<uint8_t>("observed_color", 3 * O);
    const int* observed_cloud_label = q.ptr<int32_t>("observed_label", O);
    const uint8_t* rendered_cloud_color = q.ptr<uint8_t>("rendered_color", 3 * P);
    const int* cloud_pose_map = q.ptr<int32_t>("rendered_pose_map", P);
    const int* poses_occluded = q.ptr<int32_t>("pose_occluded", num_images);
    const int* poses_label = q.ptr<int32_t>("pose_label", num_images);
    const float* observed_points_total = q.ptr<float>("pose_observed_total", num_images);
    const float* dist = q.ptr<float>("knn_dist", P);
    const int* index = q.ptr<int32_t>("knn_index", P);
    for (size_t i = 0; i < P; i++) {
        if (cloud_pose_map[i] < 0 || cloud_pose_map[i] >= num_images) throw std::runtime_error("rendered_pose_map out of range");
        if (index[i] < -1 || index[i] >= observed_cloud_point_count) throw std::runtime_error("knn_index out of range");
        if (index[i] == -1 && dist[i] <= sensor_resolution) throw std::runtime_error("a matched point without a neighbour");
    }

    // :319-330
    std::vector<float> rendered_cost(num_images, 0), pose_point_num(num_images, 0), rendered_explained(num_images, 0);
    std::vector<uint8_t> observed_explained((size_t)num_images * O, 0);
    const int* cuda_observed_cloud_label = (cost_type == 2) ? observed_cloud_label : nullptr;
    // :343-360
    blockDim.x = THREADS_PER_BLOCK;
    blockDim.y = 1;
    blockIdx.y = threadIdx.y = 0;
    gridDim.x = (unsigned)((rendered_cloud_point_count + THREADS_PER_BLOCK - 1) / THREADS_PER_BLOCK);
    for (unsigned b = 0; b < gridDim.x; b++)
        for (unsigned t = 0; t < blockDim.x; t++) {
            blockIdx.x = b;
            threadIdx.x = t;
            cuda_renderer::cost_computation::compute_render_cost(
                dist, index, cloud_pose_map, poses_occluded, rendered_cost.data(), sensor_resolution, rendered_cloud_point_count,
                observed_cloud_point_count, pose_point_num.data(), rendered_cloud_color, observed_cloud_color,
                data_of(observed_explained), poses_label, cuda_observed_cloud_label, cost_type, color_distance_threshold);
        }
    // :362-378 the percentage chain
    const std::vector<float> percentage_multiplier_val(num_images, 100);
    const cuda_renderer::cost_computation::cost_percentage_functor percentage;
    const cuda_renderer::cost_computation::cost_multiplier_functor multiplier;
    for (int i = 0; i < num_images; i++) rendered_explained[i] = pose_point_num[i] - rendered_cost[i];            // :364-368 minus
    for (int i = 0; i < num_images; i++) rendered_cost[i] = percentage(rendered_cost[i], pose_point_num[i]);      // :369-373
    for (int i = 0; i < num_images; i++) rendered_cost[i] = multiplier(rendered_cost[i], percentage_multiplier_val[i]);  // :374-378
    out.put("rendered_cost", rendered_cost, {num_images});
    out.put("pose_point_num", pose_point_num, {num_images});
    if (calculate_observed_cost) {  // :387-455
        std::vector<float> pose_observed_explained(num_images, 0), points_diff(num_images, 0), observed_cost(num_images, 0);
        gridDim.x = (unsigned)(((size_t)num_images * O + THREADS_PER_BLOCK - 1) / THREADS_PER_BLOCK);
        for (unsigned b = 0; b < gridDim.x; b++)
            for (unsigned t = 0; t < blockDim.x; t++) {  // :399-404
                blockIdx.x = b;
                threadIdx.x = t;
                cuda_renderer::cost_computation::compute_observed_cost(num_images, observed_cloud_point_count,
                                                                       data_of(observed_explained), pose_observed_explained.data());
            }
        for (int i = 0; i < num_images; i++) points_diff[i] = rendered_explained[i] - pose_observed_explained[i];       // :407-411
        for (int i = 0; i < num_images; i++) observed_cost[i] = observed_points_total[i] - pose_observed_explained[i];  // :422-426
        for (int i = 0; i < num_images; i++) observed_cost[i] = observed_cost[i] / observed_points_total[i];            // :435-439
        for (int i = 0; i < num_images; i++) observed_cost[i] = observed_cost[i] * percentage_multiplier_val[i];        // :442-446
        out.put("observed_cost", observed_cost, {num_images});
        out.put("points_diff_cost", points_diff, {num_images});
    }
}

// ---- rgb2lab and color_distance (compute_costs.cuh:57-159), argument for argument -----------------------------
void run_colour(const Bundle& q, Bundle& out) {
    const size_t n = q.count("rgb") / 3, m = q.count("lab_pairs") / 6;
    const uint8_t* rgb = q.ptr<uint8_t>("rgb", 3 * n);
    const float* pairs = q.ptr<float>("lab_pairs", 6 * m);
    std::vector<float> lab(3 * n);
    for (size_t i = 0; i < n; i++) cuda_renderer::cost_computation::rgb2lab(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2], &lab[3 * i]);
    std::vector<double> dist(m);
    for (size_t i = 0; i < m; i++) {
        const float* p = pairs + 6 * i;
        dist[i] = cuda_renderer::cost_computation::color_distance(p[0], p[1], p[2], p[3], p[4], p[5]);
    }
    out.put("lab", lab, {(int64_t)n, 3});
    out.put("distance", dist, {(int64_t)m});
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s <request> <result>\n", argv[0]);
        return 2;
    }
    try {
        const Bundle q = read_bundle(argv[1]);
        Bundle out;
        const int op = q.geti("op");
        if (op == 1) {  // render in both triangle orders, then the cloud of the ascending render when a stride is given
            std::vector<int32_t> depth;
            std::vector<uint8_t> rgb;
            run_render(q, out, false, "", &depth, &rgb);
            run_render(q, out, true, "_desc", nullptr, nullptr);
            if (q.has("stride")) run_cloud(q, out, depth.data(), rgb.data(), (int)(q.count("poses") / 16), "cloud_");
        } else if (op == 2) {  // the cloud of given depth images and colour planes (depth2cloud_global, renderer.cu:1936-2069)
            const size_t n = q.count("depth");
            const int num_poses = (int)(n / ((size_t)q.geti("width") * q.geti("height")));
            run_cloud(q, out, q.ptr<int32_t>("depth"), q.ptr<uint8_t>("planes", 3 * n), num_poses, "cloud_");
        } else if (op == 3) {
            run_costs(q, out);
        } else if (op == 4) {
            run_colour(q, out);
        } else {
            throw std::runtime_error("unknown op");
        }
        write_bundle(argv[2], out);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ref_host: %s\n", e.what());
        return 1;
    }
    return 0;
}
