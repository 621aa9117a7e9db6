// Stand-alone host check of posendf_amd/csrc/pndf_lbs_pack.h (no HIP, no library): the packers behind pndf_lbs_pack_host and
// pndf_lbs_pack_split_host and the picked-joint table of pndf_lbs_create, on three small synthetic models.  Every buffer is a
// heap allocation of exactly the size the packers are documented to take, so the same program under
// -fsanitize=address,undefined is the out-of-bounds check.  Exit status 0 and one "ok" line, or the first failures and 1.
// Built and run by tests/test_lbs_pack_host.py.
#include <cstdio>
#include <cstdlib>

#include "pndf_lbs_pack.h"

using namespace pndf_lbs;

static int failures = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        if (!(cond)) {                                            \
            if (++failures <= 20) {                               \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__);  \
                std::printf(__VA_ARGS__);                         \
                std::printf("\n");                                \
            }                                                     \
        }                                                         \
    } while (0)

// ---- a small deterministic generator (64-bit LCG, the high bits)
struct Rng {
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed * 2862933555777941757ull + 3037000493ull) {}
    uint32_t u32() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(s >> 32);
    }
    float unit() { return (float)(u32() >> 8) * (1.0f / 16777216.0f); }      // [0, 1)
    // +-[lo, 1) * scale: every entry within a factor 1 / lo of the largest, see check_split
    float signed_in(float lo, float scale) { return ((u32() & 1u) ? -1.0f : 1.0f) * (lo + (1.0f - lo) * unit()) * scale; }
};

struct Model {
    int V = 0, NB = 0;
    std::vector<float> v_template, shapedirs, betas, posedirs, J_regressor, lbs_weights;
    std::vector<int32_t> parents, extra;
};

static const int32_t SMPL_TREE[NJ] = {-1, 0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 9, 12, 13, 14, 16, 17, 18, 19, 20, 21};
// a chain with two side branches (tests/test_lbs_gpu.py: test_other_kinematic_tree_takes_the_generic_per_frame_kernels)
static const int32_t OTHER_TREE[NJ] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 3, 20, 7, 22};

static Model make_model(int V, int NB, const int32_t* tree, std::vector<int32_t> extra, uint64_t seed) {
    Rng r(seed);
    Model m;
    m.V = V;
    m.NB = NB;
    m.parents.assign(tree, tree + NJ);
    m.extra = std::move(extra);
    m.v_template.resize((size_t)V * 3);
    for (float& x : m.v_template) x = r.signed_in(0.05f, 1.0f);
    m.shapedirs.resize((size_t)V * 3 * NB);
    for (float& x : m.shapedirs) x = r.signed_in(0.05f, 0.03f);
    m.betas.resize(NB);
    for (float& x : m.betas) x = r.signed_in(0.05f, 2.0f);
    m.posedirs.resize((size_t)9 * (NJ - 1) * V * 3);
    for (float& x : m.posedirs) x = r.signed_in(0.05f, 0.01f);
    m.J_regressor.assign((size_t)NJ * V, 0.f);
    for (int j = 0; j < NJ; ++j) {      // each joint: the mean of four vertices
        for (int k = 0; k < 4; ++k) m.J_regressor[(size_t)j * V + r.u32() % (uint32_t)V] += 0.25f;
    }
    m.lbs_weights.assign((size_t)V * NJ, 0.f);
    for (int v = 0; v < V; ++v) {       // each vertex: up to three joints, weights in [0.1, 0.8], summing to 1
        const float w0 = 0.1f + 0.3f * r.unit(), w1 = 0.1f + 0.3f * r.unit();
        const int j0 = (int)(r.u32() % NJ), j1 = (j0 + 1 + (int)(r.u32() % 5)) % NJ, j2 = (j1 + 6 + (int)(r.u32() % 5)) % NJ;
        m.lbs_weights[(size_t)v * NJ + j0] += w0;
        m.lbs_weights[(size_t)v * NJ + j1] += w1;
        m.lbs_weights[(size_t)v * NJ + j2] += 1.0f - w0 - w1;
    }
    return m;
}

static const float* ptr(const std::vector<float>& v) { return v.empty() ? nullptr : v.data(); }

static int pack(const Model& m, float* blob, float* J, float* rel) {
    return lbs_pack(m.V, m.NB, m.v_template.data(), ptr(m.shapedirs), ptr(m.betas), m.posedirs.data(), m.J_regressor.data(),
                    m.parents.data(), m.lbs_weights.data(), m.extra.empty() ? nullptr : m.extra.data(), (int32_t)m.extra.size(), blob, J, rel);
}

// ---- 1. the picked-joint table from the blob == the table pndf_lbs_create used to build from the model arrays
static void check_picked(const Model& m, const std::vector<float>& blob) {
    const int NE = (int)m.extra.size(), npf = 9 * (NJ - 1);
    std::vector<float> got((size_t)NE * PICK_FLOATS, -7.f), want((size_t)NE * PICK_FLOATS);
    lbs_picked_table(blob.data(), m.extra.data(), NE, got.data());
    for (int x = 0; x < NE; ++x) {
        const int v = m.extra[x];
        float* P = want.data() + (size_t)x * PICK_FLOATS;
        for (int c = 0; c < 3; ++c) {
            double acc = m.v_template[(size_t)v * 3 + c];
            for (int l = 0; l < m.NB; ++l) acc += (double)m.shapedirs[((size_t)v * 3 + c) * m.NB + l] * m.betas[l];
            P[c] = (float)acc;
        }
        for (int j = 0; j < NJ; ++j) P[3 + j] = m.lbs_weights[(size_t)v * NJ + j];
        for (int k = 0; k < npf; ++k)
            for (int c = 0; c < 3; ++c) P[3 + NJ + 3 * k + c] = m.posedirs[(size_t)k * m.V * 3 + (size_t)v * 3 + c];
    }
    CHECK(NE == 0 || memcmp(got.data(), want.data(), want.size() * sizeof(float)) == 0, "V = %d: picked table differs", m.V);
}

// ---- 2. hi + lo of every packed P and W entry reproduces x * scale to 2^-21 relative
// Two round-to-nearest fp16 steps leave at most 2^-11 * 2^-11 = 2^-22 of x; one more bit for a lo half that is subnormal
// (quantum 2^-24 instead of its own last place).  The largest entry sits in [2^12, 2^13) after scaling and the generator keeps
// every non-zero entry within 2^-5 of it, so a lo half never falls below what the subnormal quantum can carry.
static double check_split(const Model& m, const std::vector<float>& blob) {
    const int NG = (m.V + GV - 1) / GV;
    const size_t bytes = (size_t)NG * PNDF_LBS_SB_BYTES;
    uint8_t* sblob = (uint8_t*)std::malloc(bytes);      // exactly sized
    float scales[2] = {0.f, 0.f};
    CHECK(lbs_pack_split_host(m.V, blob.data(), sblob, scales) == PNDF_OK, "V = %d: split pack refused", m.V);
    CHECK(scales[0] > 0.f && scales[1] > 0.f, "V = %d: scales %g %g", m.V, scales[0], scales[1]);
    double worst = 0.0;
    auto entry = [&](const uint8_t* o, int hi_off, int lo_off, int row, int vi, float x, float scale, const char* what) {
        uint16_t h, l;
        memcpy(&h, o + hi_off + pndf_lbs_sb_at(row, vi), 2);
        memcpy(&l, o + lo_off + pndf_lbs_sb_at(row, vi), 2);
        const double y = (double)x * scale, err = std::fabs((double)f16_to_f32(h) + (double)f16_to_f32(l) - y);
        const double rel = y != 0.0 ? err / std::fabs(y) : err;
        if (rel > worst) worst = rel;
        CHECK(rel <= std::ldexp(1.0, -21), "V = %d %s row %d vertex %d: %.9g -> hi + lo off by %.3g relative", m.V, what, row, vi, y, rel);
    };
    for (int grp = 0; grp < NG; ++grp) {
        const float* b = blob.data() + (size_t)grp * BLOB;
        const uint8_t* o = sblob + (size_t)grp * PNDF_LBS_SB_BYTES;
        for (int c = 0; c < 3; ++c)
            for (int k = 0; k < PF; ++k)
                for (int vi = 0; vi < GV; ++vi)
                    entry(o, PNDF_LBS_SB_PH + c * PNDF_LBS_SB_PLANE, PNDF_LBS_SB_PL + c * PNDF_LBS_SB_PLANE, k, vi,
                          b[PNDF_LBS_BLOB_P + c * C_STRIDE + k * GV + vi], scales[0], "P");
        for (int j = 0; j < 32; ++j)
            for (int vi = 0; vi < GV; ++vi)
                entry(o, PNDF_LBS_SB_WH, PNDF_LBS_SB_WL, j, vi, b[PNDF_LBS_BLOB_W + j * GV + vi], scales[1], "W");
        CHECK(memcmp(o + PNDF_LBS_SB_VS, b + PNDF_LBS_BLOB_VS, 3 * GV * 4) == 0 && memcmp(o + PNDF_LBS_SB_FL, b + PNDF_LBS_BLOB_FL, GV * 4) == 0,
              "V = %d group %d: shaped template / flags are not copies", m.V, grp);
    }
    std::free(sblob);
    return worst;
}

// ---- 3. f32_to_f16 against the compiler's conversion
static uint16_t bits_of(_Float16 h) {
    uint16_t b;
    memcpy(&b, &h, 2);
    return b;
}
static bool is_nan16(uint16_t b) { return (b & 0x7c00u) == 0x7c00u && (b & 0x3ffu) != 0; }
static void same_half(float f, const char* what) {
    const uint16_t got = f32_to_f16(f), want = bits_of((_Float16)f);
    CHECK(got == want || (is_nan16(got) && is_nan16(want)), "%s: f32_to_f16(%.9g) = 0x%04x, the compiler says 0x%04x", what, f, got, want);
}
static int check_f16() {
    int cases = 0;
    for (uint32_t b = 0; b < 65536u; ++b, ++cases) {      // every half -> float -> half is the identity
        const uint16_t h = (uint16_t)b;
        _Float16 x;
        memcpy(&x, &h, 2);
        const float f = (float)x;
        const uint16_t back = f32_to_f16(f);
        CHECK(back == h || (is_nan16(h) && is_nan16(back)), "half 0x%04x -> %.9g -> 0x%04x", h, f, back);
        if ((h & 0x7c00u) != 0x7c00u) CHECK(f16_to_f32(h) == f, "f16_to_f32(0x%04x) = %.9g, the compiler says %.9g", h, f16_to_f32(h), f);
    }
    for (uint32_t b = 0; b < 0x7c00u; ++b) {              // midpoints of neighbouring halfs (ties to even), and one float either side
        const uint16_t h0 = (uint16_t)b, h1 = (uint16_t)(b + 1);
        // (0x7bff's neighbour is infinity: the midpoint that rounds there is 65520 = 65504 + half a last place)
        const double lo = f16_to_f32(h0), hi = (h1 == 0x7c00u) ? 65536.0 : (double)f16_to_f32(h1);
        const float mid = (float)((lo + hi) * 0.5);
        for (float s : {1.0f, -1.0f})
            for (float f : {mid, std::nextafter(mid, 0.0f), std::nextafter(mid, 1e30f)}) {
                same_half(s * f, "midpoint");
                ++cases;
            }
    }
    for (float f : {0.0f, -0.0f, 65504.0f, 65519.996f, 65520.0f, 1e30f, -1e30f, INFINITY, -INFINITY, NAN, 1e-30f, 5.9604645e-8f, 2.9802322e-8f}) {
        same_half(f, "special");
        ++cases;
    }
    return cases;
}

// ---- 4. the refusals: their codes, and nothing written
static bool all_bytes(const void* p, size_t n, uint8_t v) {
    const uint8_t* b = (const uint8_t*)p;
    for (size_t i = 0; i < n; ++i)
        if (b[i] != v) return false;
    return true;
}
static int check_refusals(const Model& good) {
    const int NG = (good.V + GV - 1) / GV;
    const size_t blob_bytes = (size_t)NG * BLOB * sizeof(float), sb_bytes = (size_t)NG * PNDF_LBS_SB_BYTES;
    float* blob = (float*)std::malloc(blob_bytes);
    uint8_t* sblob = (uint8_t*)std::malloc(sb_bytes);
    float J[NJ * 3], rel[NJ * 3], scales[2];
    int cases = 0;
    auto arm = [&]() {
        memset(blob, 0xA5, blob_bytes);
        memset(sblob, 0xA5, sb_bytes);
        memset(J, 0xA5, sizeof(J));
        memset(rel, 0xA5, sizeof(rel));
        memset(scales, 0xA5, sizeof(scales));
    };
    auto untouched = [&]() {
        return all_bytes(blob, blob_bytes, 0xA5) && all_bytes(sblob, sb_bytes, 0xA5) && all_bytes(J, sizeof(J), 0xA5) &&
               all_bytes(rel, sizeof(rel), 0xA5) && all_bytes(scales, sizeof(scales), 0xA5);
    };
    auto refuse = [&](const Model& m, int want, const char* what) {
        arm();
        const int rc = pack(m, blob, J, rel);
        CHECK(rc == want, "%s: returned %d, expected %d", what, rc, want);
        CHECK(untouched(), "%s: a refusal wrote to its outputs", what);
        ++cases;
    };
    Model m = good;
    m.parents[5] = 7;      // a parent after its child
    refuse(m, PNDF_ERR_UNSUPPORTED, "parent after its child");
    m = good;
    m.parents[0] = 0;
    refuse(m, PNDF_ERR_UNSUPPORTED, "a root with a parent");
    m = good;
    m.extra[1] = good.V;
    refuse(m, PNDF_ERR_BAD_ARG, "picked vertex == V");
    m.extra[1] = -1;
    refuse(m, PNDF_ERR_BAD_ARG, "picked vertex < 0");
    m = good;
    m.extra[2] = m.extra[0];
    refuse(m, PNDF_ERR_BAD_ARG, "picked vertex named twice");
    m = good;
    m.extra.clear();
    for (int e = 0; e < PNDF_LBS_MAX_EXTRA + 1; ++e) m.extra.push_back(e);
    refuse(m, PNDF_ERR_BAD_ARG, "33 picked vertices");
    m = good;
    m.V = 0;
    refuse(m, PNDF_ERR_BAD_ARG, "V = 0");
    // null pointers, one at a time
    const int32_t ne = (int32_t)good.extra.size();
    const float *vt = good.v_template.data(), *sd = good.shapedirs.data(), *be = good.betas.data(), *pd = good.posedirs.data(),
                *jr = good.J_regressor.data(), *lw = good.lbs_weights.data();
    const int32_t *pa = good.parents.data(), *ex = good.extra.data();
    auto null_case = [&](int rc, const char* what) {
        CHECK(rc == PNDF_ERR_BAD_ARG, "null %s: returned %d", what, rc);
        CHECK(untouched(), "null %s: a refusal wrote to its outputs", what);
        ++cases;
    };
    arm();
    null_case(lbs_pack(good.V, good.NB, nullptr, sd, be, pd, jr, pa, lw, ex, ne, blob, J, rel), "v_template");
    null_case(lbs_pack(good.V, good.NB, vt, nullptr, be, pd, jr, pa, lw, ex, ne, blob, J, rel), "shapedirs");
    null_case(lbs_pack(good.V, good.NB, vt, sd, nullptr, pd, jr, pa, lw, ex, ne, blob, J, rel), "betas");
    null_case(lbs_pack(good.V, good.NB, vt, sd, be, nullptr, jr, pa, lw, ex, ne, blob, J, rel), "posedirs");
    null_case(lbs_pack(good.V, good.NB, vt, sd, be, pd, nullptr, pa, lw, ex, ne, blob, J, rel), "J_regressor");
    null_case(lbs_pack(good.V, good.NB, vt, sd, be, pd, jr, nullptr, lw, ex, ne, blob, J, rel), "parents");
    null_case(lbs_pack(good.V, good.NB, vt, sd, be, pd, jr, pa, nullptr, ex, ne, blob, J, rel), "lbs_weights");
    null_case(lbs_pack(good.V, good.NB, vt, sd, be, pd, jr, pa, lw, nullptr, ne, blob, J, rel), "extra_joint_vertex");
    null_case(lbs_pack(good.V, good.NB, vt, sd, be, pd, jr, pa, lw, ex, ne, nullptr, J, rel), "blob");
    null_case(lbs_pack(good.V, -1, vt, sd, be, pd, jr, pa, lw, ex, ne, blob, J, rel), "(NB < 0)");
    null_case(lbs_pack(good.V, good.NB, vt, sd, be, pd, jr, pa, lw, ex, -1, blob, J, rel), "(n_extra < 0)");
    // the split packer (its input is a blob: the sentinel bytes serve)
    null_case(lbs_pack_split_host(good.V, nullptr, sblob, scales), "blob (split)");
    null_case(lbs_pack_split_host(good.V, blob, nullptr, scales), "sblob");
    null_case(lbs_pack_split_host(0, blob, sblob, scales), "(split, V = 0)");
    std::free(blob);
    std::free(sblob);
    return cases;
}

int main() {
    const Model models[3] = {make_model(17, 0, SMPL_TREE, {}, 1), make_model(41, 3, SMPL_TREE, {3, 17, 40}, 2),
                             make_model(137, 2, OTHER_TREE, {5, 60, 136}, 3)};
    double worst = 0.0;
    for (const Model& m : models) {
        const int NG = (m.V + GV - 1) / GV;
        std::vector<float> blob((size_t)NG * BLOB, -3.f), J(NJ * 3), rel(NJ * 3);
        const int rc = pack(m, blob.data(), J.data(), rel.data());
        CHECK(rc == PNDF_OK, "V = %d: pack returned %d", m.V, rc);
        if (rc != PNDF_OK) continue;
        check_picked(m, blob);
        const double w = check_split(m, blob);
        if (w > worst) worst = w;
    }
    const int f16_cases = check_f16();
    const int refusals = check_refusals(models[1]);
    if (failures) {
        std::printf("lbs_pack_check: %d FAILURES\n", failures);
        return 1;
    }
    std::printf("lbs_pack_check: ok -- 3 models (V = 17, 41, 137): picked tables equal bit for bit; hi + lo of P and W within %.3g = 2^%.2f "
                "relative (bound 2^-21); %d half conversions agree with the compiler; %d refusals with their codes, nothing written\n",
                worst, std::log2(worst), f16_cases, refusals);
    return 0;
}
