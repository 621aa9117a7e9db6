// Stand-alone host program (own main, no HIP, no library): the host twin's track path -- pndf_project_ex_cpu with a pndf_project_options3
// (include/posendf_amd.h) -- on a 15-joint hand with synthetic weights, three tracks of T = 5 frames, three steps, with a joint mask.
// Built with csrc/pndf_cpu.cpp in the same command; meant for a sanitizer build on the CPU,
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -pthread tests/host/skeleton_track_check.cpp
//         posendf_amd/csrc/pndf_cpu.cpp -o skeleton_track_check
// and checked without one by tests/test_skeleton_track_host.py.  Exit status 0 and one line that names what was checked.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/posendf_amd.h"

namespace {

const int32_t HAND[15] = {-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13};
constexpr int J = 15, NQ = 4 * J, P = 3, T = 5, B = P * T, STEPS = 3;

uint32_t rng_state = 12345u;
float uniform() {      // [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        printf("skeleton_track_check: FAILED %s\n", what);
        ++failures;
    }
}

bool same_bits(const float* a, const float* b, size_t n) { return memcmp(a, b, n * sizeof(float)) == 0; }

}  // namespace

int main() {
    pndf_config cfg;
    memset(&cfg, 0, sizeof(cfg));
    cfg.act = 1;      // lrelu
    cfg.beta = 100.0f;
    cfg.num_joints = J;
    const int32_t dims[4] = {6 * J, 24, 16, 1};
    cfg.n_dims = 4;
    for (int i = 0; i < 4; ++i) cfg.dims[i] = dims[i];
    for (int j = 0; j < J; ++j) cfg.parent[j] = HAND[j];
    cfg.precision = PNDF_PREC_FP32;
    cfg.enc_act = -1;
    pndf_cpu_handle h = nullptr;
    if (pndf_cpu_create(&h, &cfg) != 0) {
        printf("skeleton_track_check: pndf_cpu_create failed: %s\n", pndf_cpu_last_error(nullptr));
        return 1;
    }
    // the tensors in state-dict order: four per bone, then weight and bias of every trunk layer
    std::vector<std::vector<float>> tensors;
    auto tensor = [&](int64_t n, float scale, float shift) {
        std::vector<float> t((size_t)n);
        for (float& x : t) x = (uniform() - 0.5f) * scale + shift;
        tensors.push_back(t);
    };
    for (int j = 0; j < J; ++j) {
        const int in = HAND[j] < 0 ? 4 : 10;
        tensor(10 * in, 2.0f / sqrtf((float)in), 0.f);
        tensor(10, 0.2f, 0.f);
        tensor(6 * 10, 2.0f / sqrtf(10.f), 0.f);
        tensor(6, 0.2f, 0.f);
    }
    for (int l = 0; l < 3; ++l) {
        tensor((int64_t)dims[l + 1] * dims[l], 4.0f / sqrtf((float)dims[l]), 0.f);
        tensor(dims[l + 1], 0.2f, l == 2 ? 0.3f : 0.f);
    }
    std::vector<const float*> ptrs;
    std::vector<int64_t> numel;
    for (const auto& t : tensors) {
        ptrs.push_back(t.data());
        numel.push_back((int64_t)t.size());
    }
    if (pndf_cpu_load_weights(h, ptrs.data(), numel.data(), (int)ptrs.size()) != 0) {
        printf("skeleton_track_check: pndf_cpu_load_weights failed: %s\n", pndf_cpu_last_error(h));
        return 1;
    }
    // three tracks of five frames: unit quaternions of random sign, so the alignment of the fill has work to do
    std::vector<float> q((size_t)B * NQ), out((size_t)B * NQ, 7.0f), ref((size_t)B * NQ, 7.0f), d((size_t)B, 7.0f), dref((size_t)B, 7.0f);
    for (int i = 0; i < B * J; ++i) {
        float v[4], n = 0.f;
        for (float& x : v) {
            x = uniform() - 0.5f;
            n += x * x;
        }
        for (int c = 0; c < 4; ++c) q[(size_t)i * 4 + c] = v[c] / sqrtf(n);
    }
    // the mask: every third joint of the interior frames of track 1 is observed
    std::vector<uint32_t> words((size_t)B, 0u), ends((size_t)B, 0u);
    for (int k = 1; k < T - 1; ++k) words[(size_t)(1 * T + k)] = 0x1249u << (k % 3);
    for (int f = 0; f < B; ++f) ends[(size_t)f] = (f % T == 0 || f % T == T - 1) ? 0xFFFFFFFFu : words[(size_t)f];

    pndf_project_options3 o;
    o.base2.base.struct_size = sizeof o;      // (pndf_default_project_options lives in the device library: the defaults by hand)
    o.base2.base.step_size = 1.0f;
    o.base2.base.tol = 0.0f;
    o.base2.base.renorm = PNDF_RENORM_UNIT;
    o.base2.observed = words.data();
    o.base2.reserved = 0;
    o.frames = T;
    o.lambda = 0.5f;
    o.fill = PNDF_TRACK_SLERP;
    o.reserved2 = 0;
    const pndf_project_options* opt = (const pndf_project_options*)&o;

    // 1. the fill alone: frame 0 is a, frame T-1 is +-b, unit interior frames, zero distances
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, 0, opt) == 0, "steps = 0 runs");
    std::vector<float> start = out;
    for (int p = 0; p < P; ++p) {
        expect(same_bits(&out[(size_t)(p * T) * NQ], &q[(size_t)(p * T) * NQ], NQ), "frame 0 of the fill is a");
        for (int i = 0; i < NQ; ++i) {
            const size_t at = (size_t)(p * T + T - 1) * NQ + i;
            expect(fabsf(out[at]) == fabsf(q[at]), "frame T-1 of the fill is +-b");
        }
    }
    for (int f = 0; f < B; ++f) expect(d[(size_t)f] == 0.f, "steps = 0 zeroes d_last");
    for (int i = 0; i < B * J; ++i) {
        float n = 0.f;
        for (int c = 0; c < 4; ++c) n += out[(size_t)i * 4 + c] * out[(size_t)i * 4 + c];
        expect(fabsf(n - 1.f) < 1e-5f, "the fill is unit");
    }
    // 2. three coupled steps with the mask: end frames and observed joints keep the fill's bits, the rest moves and stays finite
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "three coupled steps run");
    int moved = 0;
    for (int f = 0; f < B; ++f)
        for (int j = 0; j < J; ++j) {
            const size_t at = ((size_t)f * J + j) * 4;
            const bool held = (ends[(size_t)f] >> j) & 1u;
            if (held) expect(same_bits(&out[at], &start[at], 4), "a held joint keeps its bits");
            else moved += !same_bits(&out[at], &start[at], 4);
            for (int c = 0; c < 4; ++c) expect(isfinite(out[at + c]), "finite poses");
        }
    expect(moved > 0, "free joints move");
    for (int f = 0; f < B; ++f) expect(isfinite(d[(size_t)f]), "finite distances");
    // 3. no coupling on the given track: the 32-byte call with all ones in the words of the end frames, bit for bit
    o.lambda = 0.f;
    o.fill = PNDF_TRACK_GIVEN;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "three uncoupled steps run");
    pndf_project_options2 o2 = o.base2;
    o2.base.struct_size = sizeof o2;
    o2.observed = ends.data();
    expect(pndf_project_ex_cpu(h, q.data(), ref.data(), dref.data(), B, STEPS, (const pndf_project_options*)&o2) == 0, "the masked call runs");
    expect(same_bits(out.data(), ref.data(), out.size()) && same_bits(d.data(), dref.data(), d.size()), "lambda 0 is the masked call");
    // 4. refusals write nothing
    std::fill(out.begin(), out.end(), 7.0f);
    o.frames = 4;      // 15 poses are no whole number of tracks of 4
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "frames"),
           "B % frames != 0 is refused");
    o.frames = T;
    o.lambda = 0.5f;
    expect(pndf_project_ex_cpu(h, q.data(), q.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "q_out"),
           "q_out == q_in is refused with tracks");
    for (float x : out) expect(x == 7.0f, "a refused call writes nothing");
    pndf_cpu_destroy(h);
    if (failures) {
        printf("skeleton_track_check: %d FAILURES\n", failures);
        return 1;
    }
    printf("skeleton_track_check: ok -- hand (15 joints), %d tracks of %d frames, %d steps, a joint mask: the fill, the coupled step, "
           "lambda 0 against the masked call bit for bit, 2 refusals\n", P, T, STEPS);
    return 0;
}
