// A C++ caller of the drop-in Optimizer::BundleAdjustment
// (include/gfslam/orbslam.h) — no Python, no torch: what a reference-side
// Tracking::CreateInitialMap links against for GlobalBundleAdjustemnt(mpMap, 20).
// Usage: ba_driver <dir> <nIterations>
// Inputs written by tests/test_initmap_dropin_gpu.py:
//   <dir>/ba_sizes.i32  nkf npts nedges
//   <dir>/ba_*.bin      one gf_ba_problem (kf_Tcw, kf_kind, kf_cam, pt_pos,
//                       edge_pt, edge_kf, edge_z, edge_is2)
// Outputs: gba_<tag>_T.f32 / _X.f32 / _out.u8 / _it.i32 for a free run (tag
// "free") and one whose stop flag is raised before the call ("stop").
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "gfslam/orbslam.h"

template <typename T>
static std::vector<T> load(const std::string& path, size_t n) {
    std::vector<T> v(n);
    std::ifstream(path, std::ios::binary).read(reinterpret_cast<char*>(v.data()), sizeof(T) * n);
    return v;
}

template <typename T>
static void store(const std::string& path, const T* p, size_t n) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    f.write(reinterpret_cast<const char*>(p), sizeof(T) * n);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int its = std::atoi(argv[2]);
    auto sz = load<int32_t>(dir + "/ba_sizes.i32", 3);
    const int nkf = sz[0], npts = sz[1], ne = sz[2];
    ORB_SLAM::Optimizer::LocalBAWindow w;
    w.kf_Tcw = load<float>(dir + "/ba_kf_Tcw.bin", (size_t)nkf * 16);
    w.kf_kind = load<uint8_t>(dir + "/ba_kf_kind.bin", nkf);
    w.kf_cam = load<float>(dir + "/ba_kf_cam.bin", (size_t)nkf * 4);
    w.pt_pos = load<float>(dir + "/ba_pt_pos.bin", (size_t)npts * 3);
    w.edge_pt = load<int32_t>(dir + "/ba_edge_pt.bin", ne);
    w.edge_kf = load<int32_t>(dir + "/ba_edge_kf.bin", ne);
    w.edge_z = load<float>(dir + "/ba_edge_z.bin", (size_t)ne * 2);
    w.edge_inv_sigma2 = load<float>(dir + "/ba_edge_is2.bin", ne);
    try {
        for (int stopped = 0; stopped < 2; stopped++) {
            ORB_SLAM::Optimizer::LocalBAWindow r = w;
            bool stop = stopped != 0;
            ORB_SLAM::Optimizer::BundleAdjustment(&r, its, &stop);
            const std::string base = dir + (stopped ? "/gba_stop" : "/gba_free");
            store(base + "_T.f32", r.kf_Tcw.data(), r.kf_Tcw.size());
            store(base + "_X.f32", r.pt_pos.data(), r.pt_pos.size());
            store(base + "_out.u8", r.edge_outlier.data(), r.edge_outlier.size());
            store(base + "_it.i32", r.iterations, 2);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "BundleAdjustment failed: %s\n", e.what());
        return 1;
    }
    return 0;
}
