// driver_icp.cpp -- runs the reference's own point-to-plane ICP sources on the host.  TEST INFRASTRUCTURE ONLY.
//
//   ref_icp <request file> <result file>
//
// cuda_icp's host sources are the reference's text, copied into oracle/_ref/src/cuda_icp/ by filter_sources.py and
// compiled with this file behind shim/ref_shim.h (its cv::Mat): scene/common.cpp (get_normal), scene/depth_scene/
// depth_scene.cpp (Scene_projective), scene/pcd_scene/pcd_scene.cpp (Scene_nn, KDTree_cpu::build_tree), icp.cpp
// (depth2cloud_cpu, transform_pcd, ICP_Point2Plane_cpu) and the headers with the two queries and thrust__pcd2Ab.
// This file only fills their arguments and writes their results down.
//
// What is NOT the reference's: eigen_slover_666.  Eigen is not available, so icp.cpp's definition is cut and the one
// below calls the oracle's restatement (orc_ref_solver666, oracle/ref_cpu_path.cpp) and records every call.  Built
// without OpenMP: the `reduction(+: reducer)` of icp.cpp:135 then adds the rows in index order.
//
// The reference's RegistrationResult has no iteration count.  Every turn of the loop that does not return calls the
// solver once, so the number of calls is the iteration at which it returned; which `return` it took follows from the
// last turn's count (the cloud is not moved after the last reduction, so the rows of the moved cloud are that turn's).
//
// The request and result files are bundle.h's.  Requests (`op`), all with width, height, fx, fy, cx, cy, depth (H x W
// int32 cm, handed over as a CV_32S image):
//   11 scene        -> proj_pcd, proj_normal (H x W x 3); nn_pcd, nn_normal (the tree's reordered buffers), nn_nodes
//   12 rows         cloud (n x 3), max_dist_diff -> per scene s in {proj, nn}: s_rows (n x 29), s_valid, s_dst_pcd,
//                   s_dst_normal (what the scene's query returned; zero where it returned none)
//   13 icp          cloud, max_dist_diff, rel_fitness, rel_rmse, max_iter -> per scene: s_T (16, row-major), s_fitness,
//                   s_rmse, s_iteration, s_exit (0 no accepted point, 1 relative criteria, 2 the extra turn), s_moved,
//                   s_solver_A (calls x 36), s_solver_b (calls x 6), s_solver_T (calls x 16)
//   14 depth2cloud  -> cloud (P x 3): depth2cloud_cpu<int32_t> at stride 1 (icp.cpp:73/96 overrun the mask otherwise)
// Scene_nn's radius is its private default, 0.01 m (pcd_scene.h:49): max_dist_diff is the projective scene's.
#include "cuda_icp/icp.h"

#include "bundle.h"

extern "C" void orc_ref_solver666(const float* A, const float* b, float* out_T);

namespace {
struct SolverCall {
    float A[36], b[6], T[16];
};
std::vector<SolverCall> g_solver_calls;
}  // namespace

namespace cuda_icp {
// icp.cpp:29-36 in the reference; here the oracle's restatement of it, recorded.
Mat4x4f eigen_slover_666(float* A, float* b) {
    SolverCall c;
    std::memcpy(c.A, A, sizeof c.A);
    std::memcpy(c.b, b, sizeof c.b);
    orc_ref_solver666(A, b, c.T);
    g_solver_calls.push_back(c);
    return Mat4x4f(c.T);
}
}  // namespace cuda_icp

namespace {

struct Scenes {
    Mat3x3f K;
    cv::Mat depth;
    std::vector<Vec3f> pcd_buffer, normal_buffer;
    Scene_projective projective;
    KDTree_cpu kdtree;
    Scene_nn nn;
    bool has_nn = false;
    int width = 0, height = 0;
};

void make_scenes(const Bundle& q, Scenes& s, float max_dist_diff) {
    s.width = q.geti("width");
    s.height = q.geti("height");
    if (s.width <= 0 || s.height <= 0) throw std::runtime_error("width and height must be positive");
    const int32_t* depth = q.ptr<int32_t>("depth", (size_t)s.width * s.height);
    s.K[0][0] = q.getf("fx");
    s.K[0][2] = q.getf("cx");
    s.K[1][1] = q.getf("fy");
    s.K[1][2] = q.getf("cy");
    s.K[2][2] = 1.0f;
    s.depth = cv::Mat(s.height, s.width, CV_32S);
    bool any = false;
    for (int r = 0; r < s.height; r++)
        for (int c = 0; c < s.width; c++) {
            const int32_t v = depth[(size_t)r * s.width + c];
            s.depth.at<int32_t>(r, c) = v;
            any = any || cv::saturate_cast<ushort>(v) > 0;
        }
    s.projective.init_Scene_projective_cpu(s.depth, s.K, s.pcd_buffer, s.normal_buffer, (size_t)s.width, (size_t)s.height,
                                           max_dist_diff);
    // KDTree_cpu::build_tree asserts a non-empty cloud (pcd_scene.cpp:49); an image without depth has no such scene
    s.has_nn = any;
    if (any) s.nn.init_Scene_nn_cpu(s.depth, s.K, s.kdtree);
}

void put_vec3(Bundle& out, const std::string& name, const std::vector<Vec3f>& v, std::vector<int64_t> shape) {
    std::vector<float> flat(3 * v.size());
    for (size_t i = 0; i < v.size(); i++) {
        flat[3 * i] = v[i].x;
        flat[3 * i + 1] = v[i].y;
        flat[3 * i + 2] = v[i].z;
    }
    out.put(name, flat, shape);
}

std::vector<Vec3f> cloud_of(const Bundle& q) {
    const size_t n = q.count("cloud") / 3;
    const float* p = q.ptr<float>("cloud", 3 * n);
    std::vector<Vec3f> cloud(n);
    for (size_t i = 0; i < n; i++) cloud[i] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
    return cloud;
}

template <class Scene>
void run_rows(const Scene& scene, const std::vector<Vec3f>& cloud, Bundle& out, const std::string& prefix) {
    const size_t n = cloud.size();
    std::vector<float> rows(29 * n);
    std::vector<int32_t> valid(n);
    std::vector<Vec3f> dst(n), normal(n);
    cuda_icp::thrust__pcd2Ab<Scene> transformer(scene);  // icp.cpp:125
    for (size_t i = 0; i < n; i++) {
        const cuda_icp::Vec29f r = transformer(cloud[i]);
        for (int k = 0; k < 29; k++) rows[29 * i + k] = r[k];
        Vec3f dst_pcd, dst_normal;
        bool ok = false;
        scene.query(cloud[i], dst_pcd, dst_normal, ok);
        if ((r[28] == 1.0f) != ok) throw std::runtime_error("the row's count and the query's valid disagree");
        valid[i] = ok ? 1 : 0;
        if (ok) {
            dst[i] = dst_pcd;
            normal[i] = dst_normal;
        }
    }
    out.put(prefix + "rows", rows, {(int64_t)n, 29});
    out.put(prefix + "valid", valid, {(int64_t)n});
    put_vec3(out, prefix + "dst_pcd", dst, {(int64_t)n, 3});
    put_vec3(out, prefix + "dst_normal", normal, {(int64_t)n, 3});
}

template <class Scene>
void run_icp(const Scene& scene, std::vector<Vec3f> cloud, const Bundle& q, Bundle& out, const std::string& prefix) {
    const int max_iter = q.geti("max_iter");
    const cuda_icp::ICPConvergenceCriteria criteria(q.getf("rel_fitness"), q.getf("rel_rmse"), max_iter);
    g_solver_calls.clear();
    const cuda_icp::RegistrationResult result = cuda_icp::ICP_Point2Plane_cpu(cloud, scene, criteria);
    const int32_t calls = (int32_t)g_solver_calls.size();
    float T[16];
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++) T[4 * i + j] = result.transformation_[i][j];
    // the last turn's count: the rows of the cloud as the loop left it
    cuda_icp::thrust__pcd2Ab<Scene> transformer(scene);
    float count = 0;
    for (const Vec3f& p : cloud) count += transformer(p)[28];
    const int32_t exit_kind = count == 0 ? 0 : (calls == max_iter ? 2 : 1);
    if (calls > max_iter) throw std::runtime_error("more solver calls than iterations");
    out.put(prefix + "T", T, {16});
    out.put(prefix + "fitness", &result.fitness_, {1});
    out.put(prefix + "rmse", &result.inlier_rmse_, {1});
    out.put(prefix + "iteration", &calls, {1});
    out.put(prefix + "exit", &exit_kind, {1});
    put_vec3(out, prefix + "moved", cloud, {(int64_t)cloud.size(), 3});
    std::vector<float> A(36 * (size_t)calls), b(6 * (size_t)calls), E(16 * (size_t)calls);
    for (int32_t c = 0; c < calls; c++) {
        std::memcpy(&A[36 * c], g_solver_calls[c].A, sizeof g_solver_calls[c].A);
        std::memcpy(&b[6 * c], g_solver_calls[c].b, sizeof g_solver_calls[c].b);
        std::memcpy(&E[16 * c], g_solver_calls[c].T, sizeof g_solver_calls[c].T);
    }
    out.put(prefix + "solver_A", A, {calls, 36});
    out.put(prefix + "solver_b", b, {calls, 6});
    out.put(prefix + "solver_T", E, {calls, 16});
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
        Scenes s;
        if (op == 11) {
            make_scenes(q, s, 0.1f);
            put_vec3(out, "proj_pcd", s.pcd_buffer, {s.height, s.width, 3});
            put_vec3(out, "proj_normal", s.normal_buffer, {s.height, s.width, 3});
            put_vec3(out, "nn_pcd", s.kdtree.pcd_buffer, {(int64_t)s.kdtree.pcd_buffer.size(), 3});
            put_vec3(out, "nn_normal", s.kdtree.normal_buffer, {(int64_t)s.kdtree.normal_buffer.size(), 3});
            const int32_t nodes = (int32_t)s.kdtree.nodes.size();
            out.put("nn_nodes", &nodes, {1});
        } else if (op == 12) {
            make_scenes(q, s, q.getf("max_dist_diff"));
            const std::vector<Vec3f> cloud = cloud_of(q);
            run_rows(s.projective, cloud, out, "proj_");
            if (s.has_nn) run_rows(s.nn, cloud, out, "nn_");
        } else if (op == 13) {
            make_scenes(q, s, q.getf("max_dist_diff"));
            const std::vector<Vec3f> cloud = cloud_of(q);
            run_icp(s.projective, cloud, q, out, "proj_");
            if (s.has_nn) run_icp(s.nn, cloud, q, out, "nn_");
        } else if (op == 14) {
            const int width = q.geti("width"), height = q.geti("height");
            const int32_t* d = q.ptr<int32_t>("depth", (size_t)width * height);
            std::vector<int32_t> depth(d, d + (size_t)width * height);
            Mat3x3f K;
            K[0][0] = q.getf("fx");
            K[0][2] = q.getf("cx");
            K[1][1] = q.getf("fy");
            K[1][2] = q.getf("cy");
            K[2][2] = 1.0f;
            const std::vector<Vec3f> cloud = cuda_icp::depth2cloud_cpu<int32_t>(depth.data(), (uint32_t)width, (uint32_t)height, K, 1, 0, 0);
            put_vec3(out, "cloud", cloud, {(int64_t)cloud.size(), 3});
        } else {
            throw std::runtime_error("unknown op");
        }
        write_bundle(argv[2], out);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "ref_icp: %s\n", e.what());
        return 1;
    }
    return 0;
}
