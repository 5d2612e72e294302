// Serial CPU restatement of the keyframe junction between tracking and local
// mapping, written from what the reference does (Tracking::NeedNewKeyFrame,
// Tracking::CreateNewKeyFrame, KeyFrame::TrackedMapPoints, the KeyFrame
// constructor from a Frame, LocalMapping::InsertKeyFrame / InterruptBA /
// SetAcceptKeyFrames) on the state words the library keeps per stream
// (tests/newkeyframe_ref.py names them). One stream at a time, no batching,
// no vector loads: a keyframe is decided, then copied slot by slot.
#include <cstdint>
#include <cstring>

namespace {

// the state words, by position
enum { SINCE, ACCEPT, STOP, NKF, ABORT, DECISION, REF, REF_MATCHES, INLIERS, SEQ, PENDING, FRAME, NWORDS = 16 };
// decision bits
enum { EVALUATED = 1, BY_STOP = 2, BY_RELOC = 4, C1A = 8, C1B = 16, C2 = 32, CREATED = 64, INTERRUPT = 128, NO_REF = 256 };

struct Header {
    int32_t stream, seq, frame_id, n;
    double timestamp;
    float Tcw[16];
};
static_assert(sizeof(Header) == 88, "header layout");
const int KP_BYTES = 28;

// The local mapper as tracking sees it: three flags.
struct Mapper {
    bool accept, stop, abort_ba;
    void interrupt_ba() { abort_ba = true; }
    void insert_keyframe() {  // the queue push, with its two side effects
        abort_ba = true;
        accept = false;  // the mapper is busy from its next loop pass on
    }
};

// Does tracking want a keyframe? Walks the tests in the order the reference
// makes them and records which were reached and how they came out.
bool need_new_keyframe(Mapper& lm, int frames_since_kf, int frames_since_reloc, int keyframes_in_map, bool have_ref,
                       int ref_tracked, int inliers, int min_frames, int max_frames, int& bits) {
    bits = EVALUATED;
    if (lm.stop) {
        bits |= BY_STOP;
        return false;
    }
    const bool just_relocalised = frames_since_reloc < max_frames;
    if (just_relocalised && keyframes_in_map > max_frames) {
        bits |= BY_RELOC;
        return false;
    }
    if (!have_ref) {  // the reference would crash here; the library answers no
        bits |= NO_REF;
        return false;
    }
    const bool idle = lm.accept;
    const bool long_ago = frames_since_kf >= max_frames;
    const bool a_while_and_idle = frames_since_kf >= min_frames && idle;
    const double ninety_percent = static_cast<double>(ref_tracked) * 0.9;
    const bool weak = static_cast<double>(inliers) < ninety_percent && inliers > 15;
    if (long_ago) bits |= C1A;
    if (a_while_and_idle) bits |= C1B;
    if (weak) bits |= C2;
    if (!(long_ago || a_while_and_idle) || !weak) return false;
    if (idle) {
        bits |= CREATED;
        return true;
    }
    lm.interrupt_ba();
    bits |= INTERRUPT;
    return false;
}

}  // namespace

extern "C" {

// The rule alone on scalars: decision bits. n_ref < 0: no reference keyframe.
int nk_rule(int since_kf, int since_reloc, int stop, int nkf, int n_ref, int inliers, int accept, int min_frames,
            int max_frames) {
    Mapper lm{accept != 0, stop != 0, false};
    int bits = 0;
    need_new_keyframe(lm, since_kf, since_reloc, nkf, n_ref >= 0, n_ref, inliers, min_frames, max_frames, bits);
    return bits;
}

// KeyFrame::TrackedMapPoints: the slots that hold a map point, bad or not.
int nk_tracked_map_points(const int32_t* slots, int n) {
    int c = 0;
    for (int i = 0; i < n; i++)
        if (slots[i] != -1) c++;
    return c;
}

// One stream's stage of one step. state [16] in and out. The graph is the
// stream's: kf_count keyframes, slot rows kf_mp[kf_off[k] .. kf_off[k + 1]).
// The frame: n keypoints (28-byte rows), descriptors, map point per keypoint,
// pose, timestamp, frame id. The outbox slot (header + rows) is written only
// when a keyframe is created, rows [0, n) only. Returns 1 when created.
int nk_stage(int32_t* state, int stream, int working, int ref, int kf_count, const int32_t* kf_off,
             const int32_t* kf_mp, int since_reloc, int frame_id, int inliers, int min_frames, int max_frames, int n,
             const uint8_t* kps, const uint8_t* desc, const int32_t* kp2mp, const float* Tcw, double timestamp,
             Header* out_hdr, uint8_t* out_kps, uint8_t* out_desc, int32_t* out_slots) {
    // a frame went by since the last keyframe
    int since = state[SINCE] < (1 << 30) ? state[SINCE] + 1 : (1 << 30);
    state[DECISION] = 0;
    state[REF] = -1;
    state[REF_MATCHES] = 0;
    state[INLIERS] = 0;
    bool create = false;
    if (working) {
        const bool have_ref = ref >= 0 && ref < kf_count;
        int tracked = 0;
        if (have_ref) tracked = nk_tracked_map_points(kf_mp + kf_off[ref], kf_off[ref + 1] - kf_off[ref]);
        const int in_map = state[NKF] == -1 ? kf_count : state[NKF];
        // a keyframe waiting in the outbox means the mapper has not taken it: it is not idle
        Mapper lm{state[ACCEPT] != 0 && state[PENDING] == 0, state[STOP] != 0, state[ABORT] != 0};
        int bits = 0;
        create = need_new_keyframe(lm, since, since_reloc, in_map, have_ref, tracked, inliers, min_frames, max_frames,
                                   bits);
        if (create) lm.insert_keyframe();
        state[DECISION] = bits;
        state[REF] = have_ref ? ref : -1;
        state[REF_MATCHES] = tracked;
        state[INLIERS] = inliers;
        state[ABORT] = lm.abort_ba ? 1 : 0;
        if (create) state[ACCEPT] = 0;
    }
    if (!create) {
        state[SINCE] = since;
        return 0;
    }
    state[SINCE] = 0;  // this frame is the last keyframe now
    state[SEQ] += 1;
    state[PENDING] = 1;
    state[FRAME] = frame_id;
    Header h;
    std::memset(&h, 0, sizeof h);
    h.stream = stream;
    h.seq = state[SEQ];
    h.frame_id = frame_id;
    h.n = n;
    h.timestamp = timestamp;
    for (int i = 0; i < 16; i++) h.Tcw[i] = Tcw[i];
    *out_hdr = h;
    for (int i = 0; i < n; i++) {
        std::memcpy(out_kps + (size_t)i * KP_BYTES, kps + (size_t)i * KP_BYTES, KP_BYTES);
        std::memcpy(out_desc + (size_t)i * 32, desc + (size_t)i * 32, 32);
        out_slots[i] = kp2mp[i];  // every match, the pose optimisation's outliers too
    }
    return 1;
}

// SetAcceptKeyFrames from the mapper's side: refused (-1) while a keyframe waits.
int nk_set_accept(int32_t* state, int flag) {
    if (flag && state[PENDING]) return -1;
    state[ACCEPT] = flag ? 1 : 0;
    return 0;
}

// The hand-over: the first max_kf waiting keyframes, streams ascending, rows
// back to back. state [B][16], the outbox [B] / [B][cap]. Returns 0, or -3 with
// nothing taken when rows_cap is too small (*nrows = the rows needed).
int nk_take(int B, int cap, int32_t* state, const Header* hdr, const uint8_t* kps, const uint8_t* desc,
            const int32_t* slots, int max_kf, int rows_cap, Header* o_hdr, uint8_t* o_kps, uint8_t* o_desc,
            int32_t* o_slots, int* nkf, int* nrows) {
    int k = 0, r = 0;
    for (int b = 0; b < B && k < max_kf; b++)
        if (state[b * NWORDS + PENDING]) {
            k++;
            r += hdr[b].n;
        }
    *nkf = 0;
    *nrows = r;
    if (r > rows_cap) return -3;
    k = 0;
    r = 0;
    for (int b = 0; b < B && k < max_kf; b++) {
        if (!state[b * NWORDS + PENDING]) continue;
        const int n = hdr[b].n;
        o_hdr[k] = hdr[b];
        std::memcpy(o_kps + (size_t)r * KP_BYTES, kps + (size_t)b * cap * KP_BYTES, (size_t)n * KP_BYTES);
        std::memcpy(o_desc + (size_t)r * 32, desc + (size_t)b * cap * 32, (size_t)n * 32);
        std::memcpy(o_slots + r, slots + (size_t)b * cap, (size_t)n * 4);
        state[b * NWORDS + PENDING] = 0;
        k++;
        r += n;
    }
    *nkf = k;
    return 0;
}

}  // extern "C"
