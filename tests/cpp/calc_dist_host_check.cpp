// tests/cpp/calc_dist_host_check.cpp -- stand-alone host program for the sanitizers (-fsanitize=address,undefined): drives the
// launcher of CalcDistByIDs (refine.hip, launch_calc_dist) on the CPU emulation of tests/hipemu -- its argument checks, the
// cut of a call into rounds of labels x queries, the kernel's own indexing (every "GPU" thread is a host thread, so the
// sanitizers see each of its loads and stores) -- and the host combine of a sharded call (include/knhip_shards.h).
// Built and run by tests/test_calc_dist.py from the emulated copy of refine.hip + tests/hipemu/emu_runtime.cpp; no GPU, nothing
// loaded into another process.  Exit status 0 and "OK" on success.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "kernels.h"
#include "knhip_shards.h"

using namespace knhip;

static int g_fail = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); \
            g_fail++;                                                 \
        }                                                             \
    } while (0)

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}
static float bf16_round(float f) {  // (any bf16-representable value will do)
    uint32_t u = bits(f) & 0xffff0000u;
    float r;
    std::memcpy(&r, &u, 4);
    return r;
}

// the steps of the kernel, restated: sequential, one rounding per operation (the file is built with -ffp-contract=off)
static float ref_dist(bool l2, const float* q, const float* y, int d) {
    float acc = 0.f;
    for (int i = 0; i < d; i++) {
        if (l2) {
            const float t = q[i] - y[i];
            acc = acc + t * t;
        } else {
            acc = acc + q[i] * y[i];
        }
    }
    return acc;
}

struct Store {
    int d = 0, rt = KN_ROW_FP32;
    int64_t n = 0;
    std::vector<float> x;        // [n][d]
    std::vector<uint4> il;       // interleaved blocks
    std::vector<int64_t> ids, col;  // sorted direct map
};

static Store make_store(int64_t n, int d, int rt, uint32_t seed) {
    Store s;
    s.d = d;
    s.rt = rt;
    s.n = n;
    std::mt19937 g(seed);
    std::uniform_real_distribution<float> u(-3.f, 3.f);
    s.x.resize((size_t)n * d);
    for (auto& v : s.x) v = rt == KN_ROW_FP32 ? u(g) : bf16_round(u(g));
    const int nchunk = row_nchunk(d, rt), cd = row_chunk_dims(rt);
    const int64_t nblk = (n + 63) / 64;
    s.il.assign((size_t)nblk * nchunk * 64, uint4{0u, 0u, 0u, 0u});
    for (int64_t r = 0; r < n; r++) {
        for (int c = 0; c < nchunk; c++) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
            for (int e = 0; e < cd && c * cd + e < d; e++) {
                const uint32_t b = bits(s.x[(size_t)r * d + c * cd + e]);
                if (rt == KN_ROW_FP32) {
                    w[e] = b;
                } else {
                    w[e >> 1] |= (b >> 16) << (16 * (e & 1));
                }
            }
            s.il[(size_t)((r >> 6) * nchunk * 64 + (int64_t)c * 64 + (r & 63))] = uint4{w[0], w[1], w[2], w[3]};
        }
    }
    // ids 10, 13, 16, ...: row r holds id 10 + 3 r, its column is r
    for (int64_t r = 0; r < n; r++) {
        s.ids.push_back(10 + 3 * r);
        s.col.push_back(r);
    }
    return s;
}

static void run_case(const Store& s, bool l2, bool aos, bool by_map, int64_t nq, int64_t nl, int64_t round_l, int64_t round_q) {
    std::mt19937 g(7);
    std::vector<float> q((size_t)nq * s.d);
    std::uniform_real_distribution<float> u(-2.f, 2.f);
    for (auto& v : q) v = u(g);
    std::vector<int64_t> labels((size_t)nl);
    int64_t want_absent = 0, first_absent = -1;
    for (int64_t j = 0; j < nl; j++) {
        const int64_t r = (int64_t)(g() % (uint32_t)s.n);
        labels[(size_t)j] = by_map ? 10 + 3 * r : r + 5;
        if (j % 37 == 11) {  // an id that is not stored: between two ids of the map / outside the row range
            labels[(size_t)j] = by_map ? 11 + 3 * r : (j % 2 ? -1 : s.n + 5 + j);
            want_absent++;
            if (first_absent < 0) first_absent = j;
        }
    }
    std::vector<float> out((size_t)nq * nl + 1, 123.f);  // (+1: a guard element behind the matrix)
    unsigned long long absent[2] = {0ull, ~0ull};
    CalcDistArgs a{};
    a.rows = aos ? static_cast<const void*>(s.x.data()) : static_cast<const void*>(s.il.data());
    a.aos = aos ? 1 : 0;
    a.idmap_ids = by_map ? s.ids.data() : nullptr;
    a.idmap_col = by_map ? s.col.data() : nullptr;
    a.ntotal = s.n;
    a.id_offset = by_map ? 0 : 5;
    a.d = s.d;
    a.nchunk = row_nchunk(s.d, s.rt);
    a.queries = q.data();
    a.nq = nq;
    a.labels = labels.data();
    a.nlabels = nl;
    a.out = out.data();
    a.out_stride = nl;
    a.count_absent = 1;
    a.nabsent = &absent[0];
    a.first_absent = &absent[1];
    CHECK(launch_calc_dist(a, l2, s.rt, nullptr, round_l, round_q) == hipSuccess);
    CHECK((int64_t)absent[0] == want_absent);
    CHECK(want_absent == 0 || (int64_t)absent[1] == first_absent);
    CHECK(out.back() == 123.f);
    int64_t bad = 0;
    for (int64_t qi = 0; qi < nq; qi++) {
        for (int64_t j = 0; j < nl; j++) {
            const int64_t lab = labels[(size_t)j];
            const int64_t r = by_map ? ((lab - 10) % 3 == 0 ? (lab - 10) / 3 : -1) : lab - 5;
            const bool here = r >= 0 && r < s.n;
            const uint32_t got = bits(out[(size_t)(qi * nl + j)]);
            const uint32_t want = here ? bits(ref_dist(l2, q.data() + qi * s.d, s.x.data() + r * s.d, s.d)) : 0xffffffffu;
            bad += got != want;
        }
    }
    CHECK(bad == 0);
}

int main() {
    // rows: fp32 interleaved (d % 4 != 0, two passes of 128 dimensions), fp32 row-major, bf16 interleaved (d % 8 != 0)
    const Store a = make_store(150, 133, KN_ROW_FP32, 1), b = make_store(130, 20, KN_ROW_FP32, 2), c = make_store(150, 21, KN_ROW_BF16, 3);
    // one launch, and rounds of one label tile x one query tile (ragged last rounds on both axes)
    for (int rounds = 0; rounds < 2; rounds++) {
        const int64_t rl = rounds ? 64 : (int64_t)1 << 22, rq = rounds ? 32 : (int64_t)1 << 19;
        run_case(a, true, false, true, 70, 200, rl, rq);
        run_case(a, false, false, false, 33, 65, rl, rq);
        run_case(b, true, true, false, 70, 200, rl, rq);
        run_case(b, false, true, true, 1, 1, rl, rq);
        run_case(c, true, false, true, 40, 129, rl, rq);
        run_case(c, false, false, true, 7, 64, rl, rq);
    }
    run_case(a, true, false, true, 9, 130, 1, 1);  // (round sizes are rounded up to whole tiles)
    // the launcher's argument checks: nothing to do; an unknown row type; row-major typed rows; COSINE without norms; bad rounds
    CalcDistArgs z{};
    CHECK(launch_calc_dist(z, true, KN_ROW_FP32, nullptr) == hipSuccess);
    z.nq = 1;
    z.nlabels = 1;
    CHECK(launch_calc_dist(z, true, 3, nullptr) == hipErrorInvalidValue);
    CHECK(launch_calc_dist(z, true, -1, nullptr) == hipErrorInvalidValue);
    z.aos = 1;
    CHECK(launch_calc_dist(z, true, KN_ROW_BF16, nullptr) == hipErrorInvalidValue);
    z.aos = 0;
    z.cos_mode = 1;
    CHECK(launch_calc_dist(z, false, KN_ROW_FP32, nullptr) == hipErrorInvalidValue);
    z.cos_mode = 0;
    CHECK(launch_calc_dist(z, true, KN_ROW_FP32, nullptr, 0, 32) == hipErrorInvalidValue);
    CHECK(launch_calc_dist(z, true, KN_ROW_FP32, nullptr, 64, -1) == hipErrorInvalidValue);
    // the host combine of a sharded call: every label held by one shard, one by none
    {
        const float A = 0.f;
        float none;
        const uint32_t ones = 0xffffffffu;
        std::memcpy(&none, &ones, 4);
        const int64_t nq = 3, nl = 5;
        std::vector<float> p0((size_t)nq * nl, none), p1((size_t)nq * nl, none), p2((size_t)nq * nl, none), out((size_t)nq * nl, A);
        for (int64_t qi = 0; qi < nq; qi++) {
            p0[(size_t)(qi * nl + 0)] = 1.f + qi;
            p1[(size_t)(qi * nl + 1)] = -0.f;
            p2[(size_t)(qi * nl + 2)] = 7.f;
            p1[(size_t)(qi * nl + 4)] = 9.f;  // (label 3: held by no shard)
        }
        const float* parts[3] = {p0.data(), p1.data(), p2.data()};
        knhip_calc_dist_combine_host(3, nq * nl, parts, out.data());
        for (int64_t qi = 0; qi < nq; qi++) {
            CHECK(out[(size_t)(qi * nl)] == 1.f + qi && bits(out[(size_t)(qi * nl + 1)]) == 0x80000000u);
            CHECK(out[(size_t)(qi * nl + 2)] == 7.f && bits(out[(size_t)(qi * nl + 3)]) == ones && out[(size_t)(qi * nl + 4)] == 9.f);
        }
        CHECK(knhip_calc_dist_first_absent_host(out.data(), nl) == 3);
        CHECK(knhip_calc_dist_first_absent_host(out.data(), 3) == -1);
        CHECK(knhip_calc_dist_first_absent_host(out.data(), 0) == -1);
    }
    if (g_fail) {
        std::printf("%d check(s) failed\n", g_fail);
        return 1;
    }
    std::printf("OK calc_dist host check\n");
    return 0;
}
