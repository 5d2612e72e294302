// Serial CPU restatement of ORBmatcher::SearchForInitialization
// (src/ORBmatcher.cc:1172-1287) over Frame's keypoint grid (src/Frame.cc:85-86,
// 100-131, 300-377) and of the gate and the state machine of
// Tracking::FirstInitialization / Tracking::Initialize (src/Tracking.cc:547-569,
// 920-946, 988-1040) without the initialiser and the map. Written from the
// reference's lines with std::vector grid cells; it shares no header with the
// library. Besides the outputs it counts the branches it took, so that a test
// can tell whether a scene exercised them.
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

const int FRAME_GRID_ROWS = 48, FRAME_GRID_COLS = 64;
const int HISTO_LENGTH = 30, TH_LOW = 50;

struct KeyPoint {  // cv::KeyPoint
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

struct Frame {
    int mnMinX, mnMaxX, mnMinY, mnMaxY;
    float mfGridElementWidthInv, mfGridElementHeightInv;
    std::vector<KeyPoint> mvKeysUn;
    const uint8_t* mDescriptors;
    std::vector<size_t> mGrid[FRAME_GRID_COLS][FRAME_GRID_ROWS];

    Frame(const int32_t bounds[4], const KeyPoint* kps, const uint8_t* desc, int n)
        : mnMinX(bounds[0]), mnMaxX(bounds[1]), mnMinY(bounds[2]), mnMaxY(bounds[3]), mvKeysUn(kps, kps + n),
          mDescriptors(desc) {
        // Frame.cc:85-86
        mfGridElementWidthInv = static_cast<float>(FRAME_GRID_COLS) / static_cast<float>(mnMaxX - mnMinX);
        mfGridElementHeightInv = static_cast<float>(FRAME_GRID_ROWS) / static_cast<float>(mnMaxY - mnMinY);
        // Frame.cc:123-131
        for (size_t i = 0; i < mvKeysUn.size(); i++) {
            int nGridPosX, nGridPosY;
            if (PosInGrid(mvKeysUn[i], nGridPosX, nGridPosY)) mGrid[nGridPosX][nGridPosY].push_back(i);
        }
    }

    // Frame.cc:367-377
    bool PosInGrid(const KeyPoint& kp, int& posX, int& posY) const {
        posX = (int)std::round((kp.x - mnMinX) * mfGridElementWidthInv);
        posY = (int)std::round((kp.y - mnMinY) * mfGridElementHeightInv);
        if (posX < 0 || posX >= FRAME_GRID_COLS || posY < 0 || posY >= FRAME_GRID_ROWS) return false;
        return true;
    }

    // Frame.cc:300-365
    std::vector<size_t> GetFeaturesInArea(const float& x, const float& y, const float& r, int minLevel,
                                          int maxLevel) const {
        std::vector<size_t> vIndices;
        vIndices.reserve(mvKeysUn.size());

        int nMinCellX = (int)std::floor((x - mnMinX - r) * mfGridElementWidthInv);
        nMinCellX = std::max(0, nMinCellX);
        if (nMinCellX >= FRAME_GRID_COLS) return vIndices;

        int nMaxCellX = (int)std::ceil((x - mnMinX + r) * mfGridElementWidthInv);
        nMaxCellX = std::min(FRAME_GRID_COLS - 1, nMaxCellX);
        if (nMaxCellX < 0) return vIndices;

        int nMinCellY = (int)std::floor((y - mnMinY - r) * mfGridElementHeightInv);
        nMinCellY = std::max(0, nMinCellY);
        if (nMinCellY >= FRAME_GRID_ROWS) return vIndices;

        int nMaxCellY = (int)std::ceil((y - mnMinY + r) * mfGridElementHeightInv);
        nMaxCellY = std::min(FRAME_GRID_ROWS - 1, nMaxCellY);
        if (nMaxCellY < 0) return vIndices;

        bool bCheckLevels = true;
        bool bSameLevel = false;
        if (minLevel == -1 && maxLevel == -1)
            bCheckLevels = false;
        else if (minLevel == maxLevel)
            bSameLevel = true;

        for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
            for (int iy = nMinCellY; iy <= nMaxCellY; iy++) {
                const std::vector<size_t>& vCell = mGrid[ix][iy];
                if (vCell.empty()) continue;
                for (size_t j = 0, jend = vCell.size(); j < jend; j++) {
                    const KeyPoint& kpUn = mvKeysUn[vCell[j]];
                    if (bCheckLevels && !bSameLevel) {
                        if (kpUn.octave < minLevel || kpUn.octave > maxLevel) continue;
                    } else if (bSameLevel) {
                        if (kpUn.octave != minLevel) continue;
                    }
                    if (std::abs(kpUn.x - x) > r || std::abs(kpUn.y - y) > r) continue;
                    vIndices.push_back(vCell[j]);
                }
            }
        }
        return vIndices;
    }
};

// ORBmatcher.cc:2384-2400
int DescriptorDistance(const uint8_t* a, const uint8_t* b) {
    int dist = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * i, 4);
        std::memcpy(&y, b + 4 * i, 4);
        unsigned int v = x ^ y;
        v = v - ((v >> 1) & 0x55555555);
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
        dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
    }
    return dist;
}

// ORBmatcher.cc:2338-2379
void ComputeThreeMaxima(std::vector<int>* histo, const int L, int& ind1, int& ind2, int& ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = (int)histo[i].size();
        if (s > max1) {
            max3 = max2;
            max2 = max1;
            max1 = s;
            ind3 = ind2;
            ind2 = ind1;
            ind1 = i;
        } else if (s > max2) {
            max3 = max2;
            max2 = s;
            ind3 = ind2;
            ind2 = i;
        } else if (s > max3) {
            max3 = s;
            ind3 = i;
        }
    }
    if (max2 < 0.1f * (float)max1) {
        ind2 = -1;
        ind3 = -1;
    } else if (max3 < 0.1f * (float)max1) {
        ind3 = -1;
    }
}

enum { C_STEALS = 0, C_FILTERED, C_RATIO_EQUAL, C_HIST_REMOVED, C_STALE, C_N };

// ORBmatcher.cc:1172-1287
int SearchForInitialization(const Frame& F1, const Frame& F2, float* vbPrevMatched, std::vector<int>& vnMatches12,
                            int windowSize, float mfNNratio, bool mbCheckOrientation, int64_t* counters) {
    int nmatches = 0;
    vnMatches12 = std::vector<int>(F1.mvKeysUn.size(), -1);

    std::vector<int> rotHist[HISTO_LENGTH];
    for (int i = 0; i < HISTO_LENGTH; i++) rotHist[i].reserve(500);
    const float factor = 1.0f / HISTO_LENGTH;

    std::vector<int> vMatchedDistance(F2.mvKeysUn.size(), INT_MAX);
    std::vector<int> vnMatches21(F2.mvKeysUn.size(), -1);

    for (size_t i1 = 0, iend1 = F1.mvKeysUn.size(); i1 < iend1; i1++) {
        KeyPoint kp1 = F1.mvKeysUn[i1];
        int level1 = kp1.octave;
        if (level1 > 0) continue;

        std::vector<size_t> vIndices2 =
            F2.GetFeaturesInArea(vbPrevMatched[2 * i1], vbPrevMatched[2 * i1 + 1], (float)windowSize, level1, level1);
        if (vIndices2.empty()) continue;

        const uint8_t* d1 = F1.mDescriptors + 32 * i1;
        int bestDist = INT_MAX;
        int bestDist2 = INT_MAX;
        int bestIdx2 = -1;

        for (std::vector<size_t>::iterator vit = vIndices2.begin(); vit != vIndices2.end(); vit++) {
            size_t i2 = *vit;
            const uint8_t* d2 = F2.mDescriptors + 32 * i2;
            int dist = DescriptorDistance(d1, d2);
            if (vMatchedDistance[i2] <= dist) {
                counters[C_FILTERED]++;
                continue;
            }
            if (dist < bestDist) {
                bestDist2 = bestDist;
                bestDist = dist;
                bestIdx2 = (int)i2;
            } else if (dist < bestDist2) {
                bestDist2 = dist;
            }
        }

        if (bestDist <= TH_LOW) {
            if (bestDist < (float)bestDist2 * mfNNratio) {
                if (vnMatches21[bestIdx2] >= 0) {
                    vnMatches12[vnMatches21[bestIdx2]] = -1;
                    nmatches--;
                    counters[C_STEALS]++;
                }
                vnMatches12[i1] = bestIdx2;
                vnMatches21[bestIdx2] = (int)i1;
                vMatchedDistance[bestIdx2] = bestDist;
                nmatches++;

                if (mbCheckOrientation) {
                    float rot = F1.mvKeysUn[i1].angle - F2.mvKeysUn[bestIdx2].angle;
                    if (rot < 0.0) rot += 360.0f;
                    int bin = (int)std::round(rot * factor);
                    if (bin == HISTO_LENGTH) bin = 0;
                    rotHist[bin].push_back((int)i1);
                }
            } else if (bestDist2 == bestDist) {
                counters[C_RATIO_EQUAL]++;
            }
        }
    }

    if (mbCheckOrientation) {
        int ind1 = -1, ind2 = -1, ind3 = -1;
        ComputeThreeMaxima(rotHist, HISTO_LENGTH, ind1, ind2, ind3);
        for (int i = 0; i < HISTO_LENGTH; i++)  // entries of queries robbed after their accept
            for (size_t j = 0; j < rotHist[i].size(); j++) counters[C_STALE] += vnMatches12[rotHist[i][j]] < 0;
        for (int i = 0; i < HISTO_LENGTH; i++) {
            if (i == ind1 || i == ind2 || i == ind3) continue;
            for (size_t j = 0, jend = rotHist[i].size(); j < jend; j++) {
                int idx1 = rotHist[i][j];
                if (vnMatches12[idx1] >= 0) {
                    vnMatches12[idx1] = -1;
                    nmatches--;
                    counters[C_HIST_REMOVED]++;
                }
            }
        }
    }

    // Update prev matched
    for (size_t i1 = 0, iend1 = vnMatches12.size(); i1 < iend1; i1++)
        if (vnMatches12[i1] >= 0) {
            vbPrevMatched[2 * i1] = F2.mvKeysUn[vnMatches12[i1]].x;
            vbPrevMatched[2 * i1 + 1] = F2.mvKeysUn[vnMatches12[i1]].y;
        }

    return nmatches;
}

}  // namespace

extern "C" {

// bounds: mnMinX, mnMaxX, mnMinY, mnMaxY. prev [n1][2] in / out, m12 [n1] out,
// counters [5]: steals, candidates skipped by vMatchedDistance, ratio
// rejections with bestDist2 == bestDist, histogram removals, stale histogram
// entries (added to). Returns nmatches.
int sir_search(const int32_t* bounds, const KeyPoint* k1, const uint8_t* d1, int n1, const KeyPoint* k2,
               const uint8_t* d2, int n2, int window, float nnratio, int check_ori, float* prev, int32_t* m12,
               int64_t* counters) {
    Frame F1(bounds, k1, d1, n1), F2(bounds, k2, d2, n2);
    std::vector<int> v;
    const int nm = SearchForInitialization(F1, F2, prev, v, window, nnratio, check_ori != 0, counters);
    for (int i = 0; i < n1; i++) m12[i] = v[i];
    return nm;
}

// Tracking::Initialize up to the initialiser (Tracking.cc:999-1017) with
// ORBmatcher(0.9, true) and SRH_WINDOW_SIZE_INIT = 100. ini_matches [n1] is
// mvIniMatches (in / out), prev mvbPrevMatched (in / out). Returns 0 when the
// initialiser is to run, 1 / 2 when mState becomes NOT_INITIALIZED for too few
// keypoints / too few matches. *nmatches as the matcher returned it (0 when it
// did not run).
int sir_initialize_gate(const int32_t* bounds, const KeyPoint* k1, const uint8_t* d1, int n1, const KeyPoint* k2,
                        const uint8_t* d2, int n2, int thres, float* prev, int32_t* ini_matches, int32_t* nmatches,
                        int64_t* counters) {
    *nmatches = 0;
    if (n2 <= thres) {
        for (int i = 0; i < n1; i++) ini_matches[i] = -1;
        return 1;
    }
    *nmatches = sir_search(bounds, k1, d1, n1, k2, d2, n2, 100, 0.9f, 1, prev, ini_matches, counters);
    if (*nmatches < thres) return 2;
    return 0;
}

// Tracking::FirstInitialization (Tracking.cc:929-945): whether the frame
// becomes the initial frame; prev [n][2] = its keypoint positions then.
int sir_first_initialization(const KeyPoint* k, int n, int thres, float* prev) {
    if (!(n > thres)) return 0;
    for (int i = 0; i < n; i++) {
        prev[2 * i] = k[i].x;
        prev[2 * i + 1] = k[i].y;
    }
    return 1;
}

}  // extern "C"
