// Stand-alone host program (own main, no HIP, no library): the host twin's root-trajectory path -- pndf_project_ex_cpu with a
// pndf_project_options9 (include/posendf_amd.h, pndf_fk_root_smooth_step of csrc/pndf_fk.h) -- on a 15-joint hand with synthetic weights,
// three tracks of T = 5 frames, K = 20 keypoints (the joints and a tip on every leaf) seen by one camera, a free root per pose coupled to
// its neighbour frames' and drawn towards an anchor.  Every buffer is exactly as long as the call reads it: a neighbour row read in front
// of the first frame or behind the last is one past an allocation.  Built with csrc/pndf_cpu.cpp in the same command; meant for a
// sanitizer build on the CPU,
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -pthread tests/host/skeleton_root_check.cpp
//         posendf_amd/csrc/pndf_cpu.cpp -o skeleton_root_check
// and checked without one by tests/test_skeleton_root_host.py.  Exit status 0 and one line that names what was checked.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/posendf_amd.h"

namespace {

const int32_t HAND[15] = {-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13};
constexpr int J = 15, NQ = 4 * J, P = 3, T = 5, B = P * T, K = J + 5;
constexpr float LAM_ROT = 0.375f, LAM_TRANS = 0.25f, MU_ROT = 0.125f, MU_TRANS = 0.0625f, NU_ROT = 0.05f, NU_TRANS = 0.1f;

uint32_t rng_state = 13579u;
float uniform() {      // [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        printf("skeleton_root_check: FAILED %s\n", what);
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
        printf("skeleton_root_check: pndf_cpu_create failed: %s\n", pndf_cpu_last_error(nullptr));
        return 1;
    }
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
        printf("skeleton_root_check: pndf_cpu_load_weights failed: %s\n", pndf_cpu_last_error(h));
        return 1;
    }
    std::vector<float> q((size_t)B * NQ);
    for (int i = 0; i < B * J; ++i) {
        float v[4], n = 0.f;
        for (float& x : v) {
            x = uniform() - 0.5f;
            n += x * x;
        }
        for (int c = 0; c < 4; ++c) q[(size_t)i * 4 + c] = v[c] / sqrtf(n);
    }
    std::vector<float> rest((size_t)J * 3), offset((size_t)K * 3, 0.f);
    std::vector<int32_t> joint((size_t)K);
    for (float& x : rest) x = 1.5f * (uniform() - 0.5f);
    for (int k = 0; k < K; ++k) joint[(size_t)k] = k < J ? k : 3 * (k - J) + 2;
    for (int i = 3 * J; i < 3 * K; ++i) offset[(size_t)i] = uniform() - 0.5f;
    std::vector<float> target((size_t)B * K * 2);
    for (int i = 0; i < B * K; ++i) {
        target[(size_t)i * 2] = 320.f + 150.f * (uniform() - 0.5f);
        target[(size_t)i * 2 + 1] = 240.f + 150.f * (uniform() - 0.5f);
    }
    // the roots: raw quaternions near the identity about five units in front of the camera; the anchor: the roots with noise, every other
    // rotation negated so that the alignment has work to do
    std::vector<float> root0((size_t)B * 7), anchor((size_t)B * 7);
    for (int f = 0; f < B; ++f) {
        float* r = &root0[(size_t)f * 7];
        r[0] = 1.5f;
        for (int c = 1; c < 4; ++c) r[c] = 0.3f * (uniform() - 0.5f);
        r[4] = 0.5f * (uniform() - 0.5f);
        r[5] = 0.5f * (uniform() - 0.5f);
        r[6] = 5.f + 0.5f * (uniform() - 0.5f);
        for (int i = 0; i < 7; ++i) anchor[(size_t)f * 7 + i] = (r[i] + 0.05f * (uniform() - 0.5f)) * ((i < 4 && f % 2 == 0) ? -1.f : 1.f);
    }

    // one call: `steps` steps from `start` with roots `rt` (in place), the 256-byte struct or (size224) the 224-byte one
    struct Result {
        std::vector<float> out, d, energy, root;
        int rc;
    };
    auto call = [&](const std::vector<float>& start, const std::vector<float>& rt, int steps, bool size224, float lam_rot, float lam_trans,
                    const float* anc, float mu_rot, float mu_trans, float nu_rot) {
        Result r{std::vector<float>((size_t)B * NQ, 7.0f), std::vector<float>((size_t)B, 7.0f), std::vector<float>((size_t)B, 7.0f), rt, 0};
        pndf_project_options9 o;
        memset(&o, 0, sizeof o);
        pndf_project_options6& o6 = o.base8.base7.base6;
        pndf_project_options5& o5 = o6.base5;
        pndf_project_options& base = o5.base4.base3.base2.base;
        base.struct_size = size224 ? sizeof(pndf_project_options8) : sizeof o;      // (pndf_default_project_options lives in the device library)
        base.step_size = 1.0f;
        base.renorm = PNDF_RENORM_UNIT;
        o5.base4.base3.frames = T;
        o5.base4.base3.lambda = 0.5f;
        o5.base4.base3.fill = PNDF_TRACK_GIVEN;
        o5.base4.flags = PNDF_TRACK_FREE_ENDS;
        o5.kp_target = target.data();
        o5.kp_energy = r.energy.data();
        o5.rest = rest.data();
        o5.kp_joint = joint.data();
        o5.kp_offset = offset.data();
        o5.n_keypoints = K;
        o5.nu = 0.1f;
        o6.root = r.root.data();
        o6.fx = 500.f; o6.fy = 480.f; o6.cx = 320.f; o6.cy = 240.f;
        o6.rho = 0.25f;
        o6.nu_rot = nu_rot;
        o6.nu_trans = NU_TRANS;
        o6.kp_flags = PNDF_KP_IMAGE;
        o.root_anchor = anc;
        o.lambda_rot = lam_rot; o.lambda_trans = lam_trans; o.mu_rot = mu_rot; o.mu_trans = mu_trans;
        r.rc = pndf_project_ex_cpu(h, start.data(), r.out.data(), r.d.data(), B, steps, (const pndf_project_options*)&o);
        return r;
    };
    auto same = [&](const Result& a, const Result& b) {
        return a.rc == 0 && b.rc == 0 && same_bits(a.out.data(), b.out.data(), a.out.size()) && same_bits(a.d.data(), b.d.data(), a.d.size()) &&
               same_bits(a.energy.data(), b.energy.data(), a.energy.size()) && same_bits(a.root.data(), b.root.data(), a.root.size());
    };

    // 1. the reduction: no coupling and no anchor is the call with the 224-byte struct, bit for bit
    for (int steps = 0; steps <= 3; ++steps)
        expect(same(call(q, root0, steps, false, 0.f, 0.f, nullptr, 0.f, 0.f, NU_ROT), call(q, root0, steps, true, 0.f, 0.f, nullptr, 0.f, 0.f, NU_ROT)),
               "lambda 0 without an anchor is the 224-byte call");

    // 2. coupled and anchored: finite, unit rotations, moved; `steps` steps are `steps` chained one-step calls bit for bit -- a one-step call
    //    ends in the second root buffer and is copied back, a two-step call ends in the caller's
    const Result three = call(q, root0, 3, false, LAM_ROT, LAM_TRANS, anchor.data(), MU_ROT, MU_TRANS, NU_ROT);
    expect(three.rc == 0, "three coupled steps run");
    if (three.rc != 0) printf("skeleton_root_check: %s\n", pndf_cpu_last_error(h));
    for (int f = 0; f < B; ++f) {
        const float* r = &three.root[(size_t)f * 7];
        bool finite = true;
        for (int i = 0; i < 7; ++i) finite = finite && isfinite(r[i]);
        expect(finite, "a coupled root is finite");
        expect(fabsf(sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]) - 1.f) < 1e-6f, "a stepped root rotation is unit");
        expect(!same_bits(r, &root0[(size_t)f * 7], 7), "a coupled root has moved");
    }
    Result chain = call(q, root0, 1, false, LAM_ROT, LAM_TRANS, anchor.data(), MU_ROT, MU_TRANS, NU_ROT);
    const Result first = chain;
    const Result two = call(q, root0, 2, false, LAM_ROT, LAM_TRANS, anchor.data(), MU_ROT, MU_TRANS, NU_ROT);
    chain = call(chain.out, chain.root, 1, false, LAM_ROT, LAM_TRANS, anchor.data(), MU_ROT, MU_TRANS, NU_ROT);
    expect(same(chain, two), "two steps are two chained one-step calls");
    chain = call(chain.out, chain.root, 1, false, LAM_ROT, LAM_TRANS, anchor.data(), MU_ROT, MU_TRANS, NU_ROT);
    expect(same(chain, three), "three steps are three chained one-step calls");

    // 3. the hand-written step of the translation: the coupled step is the uncoupled step plus lambda (0.5 (s- + s+) - s) for an interior
    //    frame, lambda 0.5 (s' - s) for an end frame, plus mu (A - s) -- each rounded on its own, so the two agree to a few ulp of the terms
    const Result plain = call(q, root0, 1, true, 0.f, 0.f, nullptr, 0.f, 0.f, NU_ROT);
    expect(plain.rc == 0, "one uncoupled step runs");
    for (int f = 0; f < B; ++f) {
        const int k = f % T;
        for (int x = 4; x < 7; ++x) {
            const float s = root0[(size_t)f * 7 + x];
            const float sm = k > 0 ? root0[(size_t)(f - 1) * 7 + x] : 0.f, sp = k < T - 1 ? root0[(size_t)(f + 1) * 7 + x] : 0.f;
            float want = plain.root[(size_t)f * 7 + x];
            if (k > 0 && k < T - 1) want += LAM_TRANS * (0.5f * (sm + sp) - s);
            else want += LAM_TRANS * (0.5f * ((k > 0 ? sm : sp) - s));
            want += MU_TRANS * (anchor[(size_t)f * 7 + x] - s);
            expect(fabsf(first.root[(size_t)f * 7 + x] - want) <= 8.f * 1.1920929e-7f * (fabsf(want) + 1.f), "the translation takes the stated step");
        }
    }
    // the poses, distances and energies of one step do not depend on the root's coupling: the term reads the root at the step's input
    expect(same_bits(first.out.data(), plain.out.data(), plain.out.size()) && same_bits(first.energy.data(), plain.energy.data(), plain.energy.size()),
           "the coupling changes only the root of a step");

    // 4. all roots of a track equal and no anchor: the coupling adds exact zeros (compared by value: +0.0 may change the sign of a zero)
    std::vector<float> equal = root0;
    for (int f = 0; f < B; ++f) memcpy(&equal[(size_t)f * 7], &root0[(size_t)(f / T) * T * 7], 7 * sizeof(float));
    const Result ec = call(q, equal, 1, false, LAM_ROT, LAM_TRANS, nullptr, 0.f, 0.f, NU_ROT), eu = call(q, equal, 1, true, 0.f, 0.f, nullptr, 0.f, 0.f, NU_ROT);
    bool equal_values = ec.rc == 0 && eu.rc == 0;
    for (size_t i = 0; i < ec.root.size(); ++i) equal_values = equal_values && ec.root[i] == eu.root[i];
    expect(equal_values, "equal roots take the uncoupled step");

    // 5. a held rotation keeps its bits and reads neither neighbours nor anchor (its part of the anchor is NaN)
    std::vector<float> half = anchor;
    for (int f = 0; f < B; ++f)
        for (int c = 0; c < 4; ++c) half[(size_t)f * 7 + c] = NAN;
    const Result held = call(q, root0, 3, false, 0.f, LAM_TRANS, half.data(), 0.f, MU_TRANS, 0.f);
    expect(held.rc == 0, "three steps with a held rotation run");
    for (int f = 0; f < B; ++f) {
        expect(same_bits(&held.root[(size_t)f * 7], &root0[(size_t)f * 7], 4), "a held rotation keeps its bits");
        expect(isfinite(held.root[(size_t)f * 7 + 4]) && isfinite(held.root[(size_t)f * 7 + 6]), "the translation beside a NaN anchor rotation is finite");
    }

    // 6. refusals write nothing
    const Result bad = call(q, root0, 1, false, 1.5f, LAM_TRANS, nullptr, 0.f, 0.f, NU_ROT);
    expect(bad.rc == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "lambda_rot") && bad.out[0] == 7.0f && same_bits(bad.root.data(), root0.data(), root0.size()),
           "a lambda outside [0, 1] is refused and nothing is written");
    const Result lone = call(q, root0, 1, false, 0.f, 0.f, anchor.data(), 0.f, 0.f, NU_ROT);
    expect(lone.rc == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "root_anchor"), "an anchor without a mu is refused");

    pndf_cpu_destroy(h);
    if (failures) return 1;
    printf("skeleton_root_check: ok (15-joint hand, %d tracks of %d frames, 20 keypoints, one camera: reduction to the 224-byte call, chained calls of both "
           "parities, the stated translation step, equal roots, a held rotation, refusals)\n", P, T);
    return 0;
}
