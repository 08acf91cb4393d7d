// Stand-alone host program for the two ring helpers of csrc/erl_common.h that sac.hip and td3.hip share: erl_ring_refusals (what an update
// entry that samples refuses about its ErlRingSample, with the code and the text the two validators wrote before they shared it) and
// erl_ring_sample_enqueue (interleaved / planar dispatch).  No GPU call is reached: the library entries the helpers name are the stubs below.
#include <stdarg.h>
#include <string.h>

#include <string>

#include "erl_common.h"

static char g_error[512];
void erl_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof g_error, fmt, ap);
    va_end(ap);
}

// S + A + 3 floats rounded up to whole 16-byte groups (include/erl_hip.h)
extern "C" int64_t erl_replay_row_floats(int S, int A) { return S >= 1 && A >= 1 ? ((int64_t)S + A + 3 + 3) / 4 * 4 : -1; }

static int g_rows_calls, g_planar_calls;
static const void *g_seen[12];
extern "C" int erl_replay_sample_rows_f32(const float *ring, int64_t max_size, int64_t num_seqs, int S, int A, const int64_t *ids, int64_t B,
                                          int64_t sample_len, float *out_state, float *out_action, float *out_reward, float *out_undone,
                                          float *out_unmask, float *out_next_state, int64_t *out_ids0, int64_t *out_ids1, void *stream)
{
    ++g_rows_calls;
    const void *seen[12] = {ring, ids, out_state, out_action, out_reward, out_undone, out_unmask, out_next_state, out_ids0, out_ids1, stream, nullptr};
    memcpy(g_seen, seen, sizeof seen);
    return max_size == 64 && num_seqs == 4 && S == 5 && A == 2 && B == 32 && sample_len == 39 ? 0 : -1;
}
extern "C" int erl_replay_sample_f32(const float *buf_states, const float *buf_actions, const float *buf_rewards, const float *buf_undones,
                                     const float *buf_unmasks, int64_t max_size, int64_t num_seqs, int S, int A, const int64_t *ids, int64_t B,
                                     int64_t sample_len, float *out_state, float *out_action, float *out_reward, float *out_undone,
                                     float *out_unmask, float *out_next_state, int64_t *out_ids0, int64_t *out_ids1, void *stream)
{
    ++g_planar_calls;
    const void *seen[12] = {buf_states, ids, out_state, out_action, out_reward, out_undone, out_unmask, out_next_state, out_ids0, out_ids1, stream, buf_unmasks};
    memcpy(g_seen, seen, sizeof seen);
    return buf_actions && buf_rewards && buf_undones && max_size == 64 && num_seqs == 4 && S == 5 && A == 2 && B == 32 && sample_len == 39 ? 0 : -1;
}

static int g_failed;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            printf("FAILED line %d: %s [%s]\n", __LINE__, #cond, g_error); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

static const int S = 5, A = 2;
static const char *const WHAT = "erl_entry_under_test";
static const std::string NULL_RING = "erl_entry_under_test: NULL ring tensor";

static bool refused(const ErlRingSample *r, bool need_ids, const std::string &text)
{
    strcpy(g_error, "untouched");
    return erl_ring_refusals(WHAT, r, need_ids, S, A) == ERL_EINVAL && text == g_error;
}
static bool accepted(const ErlRingSample *r, bool need_ids)
{
    strcpy(g_error, "untouched");
    return erl_ring_refusals(WHAT, r, need_ids, S, A) == ERL_OK && std::string("untouched") == g_error;
}
static std::string interleaved_text(long long row_floats, long long sample_len)
{
    return "erl_entry_under_test: interleaved ring with row_floats=" + std::to_string(row_floats) + " (expected 12), sample_len=" + std::to_string(sample_len);
}
static std::string shape_text(long long max_size, long long num_seqs, long long sample_len)
{
    return "erl_entry_under_test: bad ring shape max_size=" + std::to_string(max_size) + " num_seqs=" + std::to_string(num_seqs) +
           " sample_len=" + std::to_string(sample_len);
}

int main()
{
    alignas(16) static float block[64];                  // (never read: the helpers look at pointers and shapes only)
    static float planes[4][4];
    static int64_t ids[32], ids0[32], ids1[32];
    const ErlRingSample good_rows{block, nullptr, nullptr, nullptr, nullptr, 64, 4, ids, 39, ids0, ids1, 12};
    const ErlRingSample good_planar{block, planes[0], planes[1], planes[2], planes[3], 64, 4, ids, 39, ids0, ids1, 0};
    CHECK(erl_replay_row_floats(S, A) == 12);

    // ---- one good ring of each kind; a loop's ring has no ids yet (need_ids false) ----
    CHECK(accepted(&good_rows, true) && accepted(&good_planar, true));
    ErlRingSample r = good_rows;
    r.ids = nullptr;
    CHECK(accepted(&r, false) && refused(&r, true, NULL_RING));
    r = good_planar;
    r.ids = nullptr;
    CHECK(accepted(&r, false) && refused(&r, true, NULL_RING));
    r = good_rows;
    r.out_ids0 = r.out_ids1 = nullptr;                   // (may be NULL: include/erl_hip.h)
    CHECK(accepted(&r, true));

    // ---- NULL pieces ----
    CHECK(refused(nullptr, true, NULL_RING) && refused(nullptr, false, NULL_RING));
    r = good_rows;
    r.buf_states = nullptr;
    CHECK(refused(&r, true, NULL_RING));
    r = good_planar;
    r.buf_states = nullptr;
    CHECK(refused(&r, false, NULL_RING));
    for (int plane = 0; plane < 4; ++plane) {
        r = good_planar;
        (plane == 0 ? r.buf_actions : plane == 1 ? r.buf_rewards : plane == 2 ? r.buf_undones : r.buf_unmasks) = nullptr;
        CHECK(refused(&r, true, NULL_RING));
    }

    // ---- the interleaved ring's own rules: row width, 16-byte base, a next row for every sampled row ----
    r = good_rows;
    r.row_floats = 8;
    CHECK(refused(&r, true, interleaved_text(8, 39)));
    r = good_rows;
    r.buf_states = block + 1;
    CHECK(refused(&r, true, interleaved_text(12, 39)));
    r = good_rows;
    r.sample_len = 64;
    CHECK(refused(&r, true, interleaved_text(12, 64)));
    r.sample_len = 65;
    CHECK(refused(&r, true, interleaved_text(12, 65)));
    r = good_planar;                                     // (the planar ring takes sample_len == max_size and any alignment)
    r.sample_len = 64;
    r.buf_states = block + 1;
    CHECK(accepted(&r, true));

    // ---- the shape ----
    r.sample_len = 65;
    CHECK(refused(&r, true, shape_text(64, 4, 65)));
    for (const ErlRingSample &good : {good_rows, good_planar}) {
        r = good;
        r.sample_len = 0;
        CHECK(refused(&r, true, shape_text(64, 4, 0)));
        r = good;
        r.num_seqs = 0;
        CHECK(refused(&r, true, shape_text(64, 0, 39)));
        r = good;
        r.sample_len = -1;
        CHECK(refused(&r, false, shape_text(64, 4, -1)));
    }

    // ---- the dispatch: one call into the entry of the ring's kind, with the ring's fields and the six batch pointers in order ----
    static float batch[6][4];
    int stream_tag;
    CHECK(erl_ring_sample_enqueue(&good_rows, S, A, 32, batch[0], batch[1], batch[2], batch[3], batch[4], batch[5], &stream_tag) == 0);
    CHECK(g_rows_calls == 1 && g_planar_calls == 0 && g_seen[0] == block && g_seen[1] == ids && g_seen[8] == ids0 && g_seen[9] == ids1 &&
          g_seen[10] == &stream_tag);
    for (int i = 0; i < 6; ++i) CHECK(g_seen[2 + i] == batch[i]);
    CHECK(erl_ring_sample_enqueue(&good_planar, S, A, 32, batch[0], batch[1], batch[2], batch[3], batch[4], batch[5], &stream_tag) == 0);
    CHECK(g_rows_calls == 1 && g_planar_calls == 1 && g_seen[0] == block && g_seen[11] == planes[3] && g_seen[10] == &stream_tag);
    for (int i = 0; i < 6; ++i) CHECK(g_seen[2 + i] == batch[i]);
    CHECK(erl_ring_sample_enqueue(&good_rows, S, A, 31, batch[0], batch[1], batch[2], batch[3], batch[4], batch[5], nullptr) == -1);   // (the entry's code comes back)

    if (g_failed) return 1;
    printf("ring ok\n");
    return 0;
}
