// Stand-alone host program (own main, no HIP, no library): the host twin's keypoint-fitting path -- pndf_project_ex_cpu with a
// pndf_project_options5 (include/posendf_amd.h, csrc/pndf_fk.h) -- on a 15-joint hand with synthetic weights, three tracks of T = 5
// frames, three steps, K = 20 keypoints (the joints and a tip on every leaf) with confidences, a joint mask, the quaternion anchor and
// free end frames.  Built with csrc/pndf_cpu.cpp in the same command; meant for a sanitizer build on the CPU,
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -pthread tests/host/skeleton_keypoints_check.cpp
//         posendf_amd/csrc/pndf_cpu.cpp -o skeleton_keypoints_check
// and checked without one by tests/test_skeleton_keypoints_host.py.  Exit status 0 and one line that names what was checked.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/posendf_amd.h"

namespace {

const int32_t HAND[15] = {-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13};
constexpr int J = 15, NQ = 4 * J, P = 3, T = 5, B = P * T, STEPS = 3, K = J + 5;

uint32_t rng_state = 24680u;
float uniform() {      // [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        printf("skeleton_keypoints_check: FAILED %s\n", what);
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
        printf("skeleton_keypoints_check: pndf_cpu_create failed: %s\n", pndf_cpu_last_error(nullptr));
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
        printf("skeleton_keypoints_check: pndf_cpu_load_weights failed: %s\n", pndf_cpu_last_error(h));
        return 1;
    }
    // the start: three tracks of five frames, unit quaternions.  Every buffer is exactly as long as the call reads it, so a read past the
    // targets of the last pose, past a table or past the rows of the kinematics is one past an allocation
    std::vector<float> q((size_t)B * NQ), out((size_t)B * NQ, 7.0f), ref((size_t)B * NQ, 7.0f), d((size_t)B, 7.0f), dref((size_t)B, 7.0f);
    for (int i = 0; i < B * J; ++i) {
        float v[4], n = 0.f;
        for (float& x : v) {
            x = uniform() - 0.5f;
            n += x * x;
        }
        for (int c = 0; c < 4; ++c) q[(size_t)i * 4 + c] = v[c] / sqrtf(n);
    }
    // the tables: rest offsets, the joints as keypoints and a tip on every leaf (joints 2, 5, 8, 11, 14)
    std::vector<float> rest((size_t)J * 3), offset((size_t)K * 3, 0.f);
    std::vector<int32_t> joint((size_t)K);
    for (float& x : rest) x = 1.5f * (uniform() - 0.5f);
    for (int k = 0; k < K; ++k) joint[(size_t)k] = k < J ? k : 3 * (k - J) + 2;
    for (int i = 3 * J; i < 3 * K; ++i) offset[(size_t)i] = uniform() - 0.5f;
    // the detections and their confidences in (0, 1]; every seventh is missing: confidence 0, negative or NaN and a NaN target
    std::vector<float> target((size_t)B * K * 3), kconf((size_t)B * K), energy((size_t)B, 7.0f), eref((size_t)B, 7.0f);
    for (float& x : target) x = 2.0f * (uniform() - 0.5f);
    for (int i = 0; i < B * K; ++i) {
        kconf[(size_t)i] = 0.1f + 0.9f * uniform();
        if (i % 7 == 0) {
            kconf[(size_t)i] = (i % 3 == 0) ? 0.f : (i % 3 == 1) ? -1.f : NAN;
            for (int c = 0; c < 3; ++c) target[(size_t)i * 3 + c] = NAN;
        }
    }
    std::vector<float> anchor = q;
    // the mask: every third joint of every frame of track 1 is held, end frames included
    std::vector<uint32_t> words((size_t)B, 0u);
    for (int k = 0; k < T; ++k) words[(size_t)(1 * T + k)] = 0x1249u << (k % 3);

    pndf_project_options5 o;
    memset(&o, 0, sizeof o);
    pndf_project_options& base = o.base4.base3.base2.base;
    base.struct_size = sizeof o;      // (pndf_default_project_options lives in the device library: the defaults by hand)
    base.step_size = 1.0f;
    base.tol = 0.0f;
    base.renorm = PNDF_RENORM_UNIT;
    o.base4.base3.base2.observed = words.data();
    o.base4.base3.frames = T;
    o.base4.base3.lambda = 0.5f;
    o.base4.base3.fill = PNDF_TRACK_GIVEN;
    o.base4.anchor = anchor.data();
    o.base4.mu = 0.25f;
    o.base4.flags = PNDF_TRACK_FREE_ENDS;
    o.kp_target = target.data();
    o.kp_conf = kconf.data();
    o.kp_energy = energy.data();
    o.rest = rest.data();
    o.kp_joint = joint.data();
    o.kp_offset = offset.data();
    o.n_keypoints = K;
    o.nu = 0.02f;
    const pndf_project_options* opt = (const pndf_project_options*)&o;

    // 1. three fitting steps: held joints keep their bits, the others stay finite and unit; the energies are finite and positive
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "three fitting steps run");
    for (int f = 0; f < B; ++f)
        for (int j = 0; j < J; ++j) {
            const size_t at = ((size_t)f * J + j) * 4;
            if ((words[(size_t)f] >> j) & 1u) {
                expect(same_bits(&out[at], &q[at], 4), "a held joint keeps its bits");
                continue;
            }
            float n = 0.f;
            for (int c = 0; c < 4; ++c) {
                expect(isfinite(out[at + c]), "finite poses (a NaN target without confidence is not read)");
                n += out[at + c] * out[at + c];
            }
            expect(fabsf(n - 1.f) < 1e-5f, "unit quaternions");
        }
    for (int f = 0; f < B; ++f) expect(isfinite(d[(size_t)f]) && isfinite(energy[(size_t)f]) && energy[(size_t)f] > 0.f, "finite distances and energies");
    // 2. the keypoint term lowers the energy: ten steps of pure keypoints + prior end below where they started
    std::vector<float> e0((size_t)B), e1((size_t)B), mid((size_t)B * NQ);
    o.base4.base3.base2.observed = nullptr;
    o.base4.base3.frames = 0;
    o.base4.base3.lambda = 0.f;
    o.base4.anchor = nullptr;
    o.base4.mu = 0.f;
    o.base4.flags = 0;
    o.kp_energy = e0.data();
    expect(pndf_project_ex_cpu(h, q.data(), mid.data(), d.data(), B, 1, opt) == 0, "one step without tracks runs");
    o.kp_energy = e1.data();
    expect(pndf_project_ex_cpu(h, q.data(), mid.data(), d.data(), B, 10, opt) == 0, "ten steps without tracks run");
    double before = 0., after = 0.;
    for (int f = 0; f < B; ++f) {
        before += e0[(size_t)f];
        after += e1[(size_t)f];
    }
    expect(after < before, "the summed energy falls");
    // 3. in place equals out of place
    std::vector<float> inplace = q;
    o.kp_energy = eref.data();
    expect(pndf_project_ex_cpu(h, inplace.data(), inplace.data(), dref.data(), B, 10, opt) == 0, "and in place");
    expect(same_bits(mid.data(), inplace.data(), mid.size()) && same_bits(d.data(), dref.data(), d.size()) && same_bits(e1.data(), eref.data(), e1.size()),
           "in place equals out of place");
    // 4. nu = 0 and kp_target NULL are the 72-byte call, bit for bit, and zero the energies; the NaN targets are never read
    o.base4.base3.base2.observed = words.data();
    o.base4.base3.frames = T;
    o.base4.base3.lambda = 0.5f;
    o.base4.anchor = anchor.data();
    o.base4.mu = 0.25f;
    o.base4.flags = PNDF_TRACK_FREE_ENDS;
    o.kp_energy = energy.data();
    pndf_project_options4 o4 = o.base4;
    o4.base3.base2.base.struct_size = sizeof o4;
    expect(pndf_project_ex_cpu(h, q.data(), ref.data(), dref.data(), B, STEPS, (const pndf_project_options*)&o4) == 0, "the 72-byte call runs");
    o.nu = 0.f;
    for (float& x : target) x = NAN;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "nu = 0 runs");
    expect(same_bits(out.data(), ref.data(), out.size()) && same_bits(d.data(), dref.data(), d.size()), "nu 0 is the 72-byte call");
    for (float x : energy) expect(x == 0.f, "nu 0 zeroes the energies");
    o.nu = 0.02f;
    o.kp_target = nullptr;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "kp_target NULL runs");
    expect(same_bits(out.data(), ref.data(), out.size()) && same_bits(d.data(), dref.data(), d.size()), "kp_target NULL is the 72-byte call");
    // 5. refusals write nothing
    o.kp_target = target.data();
    std::fill(out.begin(), out.end(), 7.0f);
    std::fill(energy.begin(), energy.end(), 7.0f);
    o.n_keypoints = 65;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "n_keypoints"), "K = 65 is refused");
    o.n_keypoints = K;
    joint[(size_t)K - 1] = J;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "kp_joint"), "a joint out of range is refused");
    joint[(size_t)K - 1] = 14;
    o.nu = -1.f;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "nu"), "a negative nu is refused");
    o.nu = 0.02f;
    o.kp_energy = out.data();
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "kp_energy"), "energies in q_out are refused");
    for (float x : out) expect(x == 7.0f, "a refused call writes nothing");
    for (float x : energy) expect(x == 7.0f, "a refused call writes no energy");
    pndf_cpu_destroy(h);
    if (failures) {
        printf("skeleton_keypoints_check: %d FAILURES\n", failures);
        return 1;
    }
    printf("skeleton_keypoints_check: ok -- hand (15 joints), %d keypoints, %d tracks of %d frames, %d steps, a joint mask, the anchor, confidences with NaN "
           "targets and free end frames: the fitting step, the energy's fall, in place without tracks, nu 0 and kp_target NULL against the 72-byte call "
           "bit for bit, 4 refusals\n", K, P, T, STEPS);
    return 0;
}
