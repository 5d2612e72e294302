// A C++ caller of the drop-in ORBmatcher::SearchForInitialization
// (include/gfslam/orbslam.h) — no Python, no torch: what a reference-side
// Tracking::Initialize links against. It runs the matcher twice, on a second
// and then on a third frame, carrying vbPrevMatched as the tracker does while
// it stays INITIALIZING.
// Usage: searchinit_driver <dir> <window>
// Inputs written by tests/test_searchinit_dropin_gpu.py:
//   <dir>/si_sizes.i32   n1 n2 n3 mnMinX mnMaxX mnMinY mnMaxY
//   <dir>/si_k{1,2,3}.bin  keypoints (cv::KeyPoint rows)
//   <dir>/si_d{1,2,3}.bin  descriptors (32-byte rows)
// Outputs per call c in {a, b}: si_<c>_m12.i32, si_<c>_prev.f32, si_<c>_nm.i32.
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

static ORB_SLAM::Frame frame(const std::string& dir, const char* tag, int n, const int32_t* bounds) {
    ORB_SLAM::Frame F;
    F.N = n;
    F.mvKeysUn = load<ORB_SLAM::KeyPoint>(dir + "/si_k" + tag + ".bin", n);
    F.mvKeys = F.mvKeysUn;
    F.mDescriptors.rows = n;
    F.mDescriptors.data = load<uint8_t>(dir + "/si_d" + tag + ".bin", (size_t)n * 32);
    F.mnMinX = bounds[0];
    F.mnMaxX = bounds[1];
    F.mnMinY = bounds[2];
    F.mnMaxY = bounds[3];
    F.fx = F.fy = 458.f;
    F.cx = 0.5f * (bounds[0] + bounds[1]);
    F.cy = 0.5f * (bounds[2] + bounds[3]);
    return F;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string dir = argv[1];
    const int window = std::atoi(argv[2]);
    auto sz = load<int32_t>(dir + "/si_sizes.i32", 7);
    try {
        ORB_SLAM::Frame F1 = frame(dir, "1", sz[0], &sz[3]), F2 = frame(dir, "2", sz[1], &sz[3]),
                        F3 = frame(dir, "3", sz[2], &sz[3]);
        std::vector<ORB_SLAM::Point2f> prev(F1.N);
        for (int i = 0; i < F1.N; i++) prev[i] = F1.mvKeysUn[i].pt;  // Tracking::FirstInitialization
        ORB_SLAM::ORBmatcher matcher(0.9f, true);
        std::vector<int> m12;
        ORB_SLAM::Frame* cur[2] = {&F2, &F3};
        for (int c = 0; c < 2; c++) {
            const int32_t nm = matcher.SearchForInitialization(F1, *cur[c], prev, m12, window);
            const std::string base = dir + (c ? "/si_b" : "/si_a");
            std::vector<int32_t> m(m12.begin(), m12.end());
            store(base + "_m12.i32", m.data(), m.size());
            store(base + "_prev.f32", reinterpret_cast<const float*>(prev.data()), 2 * prev.size());
            store(base + "_nm.i32", &nm, 1);
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "SearchForInitialization failed: %s\n", e.what());
        return 1;
    }
    return 0;
}
