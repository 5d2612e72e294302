// CPU restatement of the relocalisation keyframe database that grows
// (gf_kfdb_create / gf_kfdb_create_growable / gf_kfdb_append / gf_kfdb_read),
// serial and written from the reference's own data structure: the inverted
// file is KeyFrameDatabase's mvInvertedFile, a list of keyframes per word that
// KeyFrameDatabase::add (KeyFrameDatabase.cc:39-45) pushes the keyframe to the
// back of for every word of its BowVector. No project header but abi.h (struct
// layouts).
//   kr_check   the verdict on a database's arrays (0, -1 GF_ERR_ARG)
//   kr_build   add() for keyframes 0 .. nkf - 1 -> the packed inverted file:
//              words ascending, a CSR of the lists
//   kr_append  the rows of new keyframes behind the packed row arrays of a
//              database held at its capacities, offsets rebased, and add() for
//              each of them in index order (0, -1, -3 GF_ERR_CAP; nothing
//              written unless 0)
#include <cstdint>
#include <cstring>
#include <list>
#include <map>
#include <vector>

#include "../../include/gfslam/abi.h"

namespace {

constexpr int KP_MAX = 4096, NKF_MAX = 64;

struct Sizes {
    int nk = 0, nb = 0, nn = 0, nf = 0;
};

int check(const gf_keyframe_db* db, Sizes& z) {
    const int nkf = db->nkf;
    if (nkf < 0) return GF_ERR_ARG;
    if (nkf == 0) return GF_OK;
    if (!db->kp_off || !db->bow_off || !db->fv_off || !db->fv_start) return GF_ERR_ARG;
    z.nk = db->kp_off[nkf];
    z.nb = db->bow_off[nkf];
    z.nn = db->fv_off[nkf];
    if (z.nn < 0) return GF_ERR_ARG;
    z.nf = db->fv_start[z.nn];
    if (z.nk < 0 || z.nb < 0 || z.nf < 0) return GF_ERR_ARG;
    for (int k = 0; k < nkf; k++) {
        const int nkp = db->kp_off[k + 1] - db->kp_off[k];
        if (db->kp_off[k] < 0 || nkp < 0 || nkp > KP_MAX) return GF_ERR_ARG;
        if (db->bow_off[k] < 0 || db->bow_off[k] > db->bow_off[k + 1]) return GF_ERR_ARG;
        if (db->fv_off[k] < 0 || db->fv_off[k] > db->fv_off[k + 1]) return GF_ERR_ARG;
        for (int e = db->bow_off[k] + 1; e < db->bow_off[k + 1]; e++)
            if (db->bow_words[e] <= db->bow_words[e - 1]) return GF_ERR_ARG;  // a std::map's keys
        for (int g = db->fv_off[k]; g < db->fv_off[k + 1]; g++) {
            if (db->fv_start[g] < 0 || db->fv_start[g] > db->fv_start[g + 1] || db->fv_start[g + 1] > z.nf)
                return GF_ERR_ARG;
            if (g > db->fv_off[k] && db->fv_nodes[g] <= db->fv_nodes[g - 1]) return GF_ERR_ARG;
            for (int x = db->fv_start[g]; x < db->fv_start[g + 1]; x++)
                if (db->fv_feats[x] < 0 || db->fv_feats[x] >= nkp) return GF_ERR_ARG;
        }
    }
    return GF_OK;
}

using Inverted = std::map<int32_t, std::list<int32_t>>;  // mvInvertedFile, sparse over the word ids

void add(Inverted& inv, const int32_t* words, int n, int kf) {
    for (int i = 0; i < n; i++) inv[words[i]].push_back(kf);  // KeyFrameDatabase.cc:43-44
}

int pack(const Inverted& inv, int32_t* inv_words, int32_t* inv_off, int32_t* inv_kf) {
    int nw = 0, at = 0;
    inv_off[0] = 0;
    for (const auto& e : inv) {
        inv_words[nw] = e.first;
        for (int32_t k : e.second) inv_kf[at++] = k;
        inv_off[++nw] = at;
    }
    return nw;
}

}  // namespace

extern "C" {

int kr_check(const gf_keyframe_db* db) {
    Sizes z;
    return check(db, z);
}

// sizes[4] = keypoints, BowVector entries, nodes, features; -> the word count, or the verdict (< 0)
int kr_build(const gf_keyframe_db* db, int32_t* inv_words, int32_t* inv_off, int32_t* inv_kf, int32_t* sizes) {
    Sizes z;
    const int rc = check(db, z);
    if (rc) return rc;
    if (db->nkf > NKF_MAX) return GF_ERR_UNSUPPORTED;
    Inverted inv;
    for (int k = 0; k < db->nkf; k++)
        add(inv, db->bow_words + db->bow_off[k], db->bow_off[k + 1] - db->bow_off[k], k);
    sizes[0] = z.nk, sizes[1] = z.nb, sizes[2] = z.nn, sizes[3] = z.nf;
    return pack(inv, inv_words, inv_off, inv_kf);
}

// st: the database's arrays at the capacities (writable despite the const of
// the shared struct), counts[6] as gf_kfdb_read gives them, in and out.
int kr_append(gf_keyframe_db* st, int32_t* inv_words, int32_t* inv_off, int32_t* inv_kf, int32_t* counts,
              const gf_keyframe_db* rows, int max_kf, int max_rows) {
    Sizes z;
    int rc = check(rows, z);
    if (rc) return rc;
    const int nkn = rows->nkf;
    if (nkn && (rows->kp_off[0] || rows->bow_off[0] || rows->fv_off[0] || rows->fv_start[0])) return GF_ERR_ARG;
    if (z.nb > z.nk || z.nn > z.nk || z.nf > z.nk) return GF_ERR_ARG;
    const int nkf0 = counts[0], nk0 = counts[1], nb0 = counts[2], nn0 = counts[3], nf0 = counts[4], nw0 = counts[5];
    if (nkf0 + nkn > max_kf || nk0 + z.nk > max_rows) return GF_ERR_CAP;
    auto I = [](const int32_t* p) { return const_cast<int32_t*>(p); };
    for (int k = 1; k <= nkn; k++) {
        I(st->kp_off)[nkf0 + k] = nk0 + rows->kp_off[k];
        I(st->bow_off)[nkf0 + k] = nb0 + rows->bow_off[k];
        I(st->fv_off)[nkf0 + k] = nn0 + rows->fv_off[k];
    }
    if (z.nk) {
        memcpy(const_cast<gf_keypoint*>(st->kps) + nk0, rows->kps, sizeof(gf_keypoint) * (size_t)z.nk);
        memcpy(const_cast<uint8_t*>(st->desc) + 32 * (size_t)nk0, rows->desc, 32 * (size_t)z.nk);
    }
    for (int e = 0; e < z.nb; e++) {
        I(st->bow_words)[nb0 + e] = rows->bow_words[e];
        const_cast<double*>(st->bow_values)[nb0 + e] = rows->bow_values[e];
    }
    for (int g = 0; g < z.nn; g++) {
        I(st->fv_nodes)[nn0 + g] = rows->fv_nodes[g];
        I(st->fv_start)[nn0 + g + 1] = nf0 + rows->fv_start[g + 1];
    }
    for (int x = 0; x < z.nf; x++) I(st->fv_feats)[nf0 + x] = rows->fv_feats[x];
    // mvInvertedFile as it stands, then add() for each new keyframe in turn
    Inverted inv;
    for (int w = 0; w < nw0; w++)
        for (int e = inv_off[w]; e < inv_off[w + 1]; e++) inv[inv_words[w]].push_back(inv_kf[e]);
    for (int k = 0; k < nkn; k++)
        add(inv, rows->bow_words + rows->bow_off[k], rows->bow_off[k + 1] - rows->bow_off[k], nkf0 + k);
    counts[0] = nkf0 + nkn;
    counts[1] = nk0 + z.nk;
    counts[2] = nb0 + z.nb;
    counts[3] = nn0 + z.nn;
    counts[4] = nf0 + z.nf;
    counts[5] = pack(inv, inv_words, inv_off, inv_kf);
    st->nkf = counts[0];
    return GF_OK;
}

}  // extern "C"
