// Stand-alone host program (own main, no HIP, no library): the host twin's bone-length path -- pndf_project_ex_cpu with a
// pndf_project_options7 (include/posendf_amd.h, the scaled term of csrc/pndf_fk.h) -- on a 15-joint hand with synthetic weights, K = 20
// keypoints (the joints and a tip on every leaf), S = 35 scales: the per-pose path (no tracks, and tracks with PNDF_LEN_PER_POSE) and the
// track path (three tracks of T = 5 frames and one of T = 70, whose sum runs over two blocks), with confidences, a joint mask, the anchor,
// free end frames, a root, rates with zeros and a clamp.  Built with csrc/pndf_cpu.cpp in the same command; meant for a sanitizer build
// on the CPU,
//   hipcc -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -pthread tests/host/skeleton_length_check.cpp
//         posendf_amd/csrc/pndf_cpu.cpp -o skeleton_length_check
// and checked without one by tests/test_skeleton_length_host.py.  Exit status 0 and one line that names what was checked.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../include/posendf_amd.h"

namespace {

const int32_t HAND[15] = {-1, 0, 1, -1, 3, 4, -1, 6, 7, -1, 9, 10, -1, 12, 13};
constexpr int J = 15, NQ = 4 * J, P = 3, T = 5, B = P * T, STEPS = 3, K = J + 5, S = J + K, LONG_T = 70;

uint32_t rng_state = 24680u;
float uniform() {      // [0, 1)
    rng_state = rng_state * 1664525u + 1013904223u;
    return (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

int failures = 0;
void expect(bool ok, const char* what) {
    if (!ok) {
        printf("skeleton_length_check: FAILED %s\n", what);
        ++failures;
    }
}

bool same_bits(const float* a, const float* b, size_t n) { return memcmp(a, b, n * sizeof(float)) == 0; }

bool all_finite(const std::vector<float>& v) {
    for (float x : v)
        if (!isfinite(x)) return false;
    return true;
}

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
        printf("skeleton_length_check: pndf_cpu_create failed: %s\n", pndf_cpu_last_error(nullptr));
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
        printf("skeleton_length_check: pndf_cpu_load_weights failed: %s\n", pndf_cpu_last_error(h));
        return 1;
    }
    // Every buffer is exactly as long as the call reads it -- the scales are [G][S] with G = P or G = B -- so a read or a write with the
    // other group count, or past the last row, is one past an allocation.  BL poses serve the long track too.
    constexpr int BL = LONG_T > B ? LONG_T : B;
    std::vector<float> q((size_t)BL * NQ), out((size_t)BL * NQ, 7.0f), ref((size_t)BL * NQ, 7.0f), d((size_t)BL, 7.0f), dref((size_t)BL, 7.0f);
    for (int i = 0; i < BL * J; ++i) {
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
    std::vector<float> target((size_t)BL * K * 3), kconf((size_t)BL * K), energy((size_t)BL, 7.0f), eref((size_t)BL, 7.0f);
    for (int i = 0; i < BL * K; ++i) {
        for (int c = 0; c < 3; ++c) target[(size_t)i * 3 + c] = 2.0f * (uniform() - 0.5f);
        kconf[(size_t)i] = 0.1f + 0.9f * uniform();
        if (i % 7 == 0) {
            kconf[(size_t)i] = (i % 3 == 0) ? 0.f : (i % 3 == 1) ? -1.f : NAN;
            for (int c = 0; c < 3; ++c) target[(size_t)i * 3 + c] = NAN;
        }
    }
    std::vector<float> root((size_t)BL * 7), root0;
    for (int f = 0; f < BL; ++f) {
        float* r = &root[(size_t)f * 7];
        r[0] = 1.5f;
        for (int c = 1; c < 4; ++c) r[c] = 0.3f * (uniform() - 0.5f);
        for (int c = 4; c < 7; ++c) r[c] = 0.2f * (uniform() - 0.5f);
    }
    root0 = root;
    std::vector<float> anchor = q;
    std::vector<uint32_t> words((size_t)BL, 0u);
    for (int k = 0; k < T; ++k) words[(size_t)(1 * T + k)] = 0x1249u << (k % 3);
    std::vector<float> rate((size_t)S);
    for (int i = 0; i < S; ++i) rate[(size_t)i] = i % 4 == 0 ? 0.f : 0.5f + uniform();
    auto scales = [&](int G) {
        std::vector<float> s((size_t)G * S);
        for (float& x : s) x = 0.8f + 0.45f * uniform();
        return s;
    };

    pndf_project_options7 o;
    memset(&o, 0, sizeof o);
    pndf_project_options6& o6 = o.base6;
    pndf_project_options5& o5 = o6.base5;
    pndf_project_options& base = o5.base4.base3.base2.base;
    base.struct_size = sizeof o;      // (pndf_default_project_options lives in the device library: the defaults by hand)
    base.step_size = 1.0f;
    base.tol = 0.0f;
    base.renorm = PNDF_RENORM_UNIT;
    o5.base4.base3.base2.observed = words.data();
    o5.base4.base3.frames = T;
    o5.base4.base3.lambda = 0.5f;
    o5.base4.base3.fill = PNDF_TRACK_GIVEN;
    o5.base4.anchor = anchor.data();
    o5.base4.mu = 0.25f;
    o5.base4.flags = PNDF_TRACK_FREE_ENDS;
    o5.kp_target = target.data();
    o5.kp_conf = kconf.data();
    o5.kp_energy = energy.data();
    o5.rest = rest.data();
    o5.kp_joint = joint.data();
    o5.kp_offset = offset.data();
    o5.n_keypoints = K;
    o5.nu = 0.02f;
    o6.root = root.data();
    o6.nu_rot = 0.02f;
    o6.nu_trans = 0.02f;
    o.len_rate = rate.data();
    o.nu_len = 0.05f;
    o.kappa = 0.1f;
    o.len_min = 0.5f;
    o.len_max = 2.0f;
    const pndf_project_options* opt = (const pndf_project_options*)&o;

    // 1. the track path: one row of scales per track [P][S]; a scale with rate 0 keeps its bits, the others move and stay in the clamp
    std::vector<float> sg = scales(P), sg0 = sg;
    o.bone_scale = sg.data();
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "three steps with one row of scales per track run");
    std::vector<float> head(out.begin(), out.begin() + (size_t)B * NQ);
    expect(all_finite(head) && all_finite(sg), "finite poses and scales (a NaN target without confidence is not read)");
    for (int g = 0; g < P; ++g)
        for (int i = 0; i < S; ++i) {
            const size_t at = (size_t)g * S + i;
            if (i % 4 == 0) expect(same_bits(&sg[at], &sg0[at], 1), "a scale with rate 0 keeps its bits");
            else expect(sg[at] != sg0[at] && sg[at] >= 0.5f && sg[at] <= 2.0f, "a scale with a positive rate moves inside the clamp");
        }
    for (int f = 0; f < B; ++f)
        for (int j = 0; j < J; ++j)
            if ((words[(size_t)f] >> j) & 1u) expect(same_bits(&out[((size_t)f * J + j) * 4], &q[((size_t)f * J + j) * 4], 4), "a held joint keeps its bits");
    // 2. tracks with PNDF_LEN_PER_POSE, and no tracks at all: one row per pose [B][S]
    root = root0;
    std::vector<float> sp = scales(B), sp0 = sp;
    o.bone_scale = sp.data();
    o.len_flags = PNDF_LEN_PER_POSE;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "three steps with one row of scales per frame run");
    expect(all_finite(sp) && !same_bits(sp.data(), sp0.data(), sp.size()), "per-frame scales move");
    o.len_flags = 0;
    o5.base4.base3.base2.observed = nullptr;
    o5.base4.base3.frames = 0;
    o5.base4.base3.lambda = 0.f;
    o5.base4.flags = 0;
    root = root0;
    sp = sp0;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "three steps without tracks run");
    std::vector<float> s_out = sp, r_out = root;
    // 3. in place equals out of place, roots and scales included
    std::vector<float> inplace(q.begin(), q.begin() + (size_t)B * NQ);
    root = root0;
    sp = sp0;
    o5.kp_energy = eref.data();
    expect(pndf_project_ex_cpu(h, inplace.data(), inplace.data(), dref.data(), B, STEPS, opt) == 0, "and in place");
    expect(same_bits(out.data(), inplace.data(), inplace.size()) && same_bits(d.data(), dref.data(), (size_t)B) && same_bits(energy.data(), eref.data(), (size_t)B) &&
               same_bits(root.data(), r_out.data(), (size_t)B * 7) && same_bits(sp.data(), s_out.data(), sp.size()),
           "in place equals out of place");
    o5.kp_energy = energy.data();
    // 4. one track of 70 frames: the sum of a group runs over a block of 64 and one of 6
    o5.base4.base3.frames = LONG_T;
    o5.base4.base3.lambda = 0.25f;
    o5.base4.flags = PNDF_TRACK_FREE_ENDS;
    o5.base4.anchor = nullptr;
    o5.base4.mu = 0.f;
    root = root0;
    std::vector<float> sl = scales(1), sl0 = sl;
    o.bone_scale = sl.data();
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), LONG_T, STEPS, opt) == 0, "a track of 70 frames runs");
    expect(all_finite(sl) && !same_bits(sl.data(), sl0.data(), sl.size()) && all_finite(out), "the long track's scales move and stay finite");
    // 5. bone_scale NULL, and ones with nu_len 0: the 168-byte call bit for bit; the ones are not written
    o5.base4.base3.frames = T;
    o5.base4.base3.lambda = 0.5f;
    o5.base4.anchor = anchor.data();
    o5.base4.mu = 0.25f;
    o5.base4.base3.base2.observed = words.data();
    pndf_project_options6 small = o6;
    small.base5.base4.base3.base2.base.struct_size = sizeof small;
    small.base5.kp_energy = eref.data();
    root = root0;
    expect(pndf_project_ex_cpu(h, q.data(), ref.data(), dref.data(), B, STEPS, (const pndf_project_options*)&small) == 0, "the 168-byte call runs");
    std::vector<float> r_small = root;
    root = root0;
    o.bone_scale = nullptr;
    o.nu_len = 0.f;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "bone_scale NULL runs");
    expect(same_bits(out.data(), ref.data(), (size_t)B * NQ) && same_bits(d.data(), dref.data(), (size_t)B) && same_bits(energy.data(), eref.data(), (size_t)B) &&
               same_bits(root.data(), r_small.data(), (size_t)B * 7),
           "bone_scale NULL is the 168-byte call");
    std::vector<float> ones((size_t)P * S, 1.0f), ones0 = ones;
    root = root0;
    o.bone_scale = ones.data();
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "scales of one with nu_len 0 run");
    expect(same_bits(out.data(), ref.data(), (size_t)B * NQ) && same_bits(energy.data(), eref.data(), (size_t)B) && same_bits(root.data(), r_small.data(), (size_t)B * 7) &&
               same_bits(ones.data(), ones0.data(), ones.size()),
           "scales of one with nu_len 0 are the 168-byte call, unwritten");
    // 6. nu = 0: the 72-byte call, and scales full of NaN are neither read nor written
    pndf_project_options4 o4 = o5.base4;
    o4.base3.base2.base.struct_size = sizeof o4;
    expect(pndf_project_ex_cpu(h, q.data(), ref.data(), dref.data(), B, STEPS, (const pndf_project_options*)&o4) == 0, "the 72-byte call runs");
    std::vector<float> nan_scale((size_t)P * S, NAN), nan_copy = nan_scale;
    o.bone_scale = nan_scale.data();
    o.nu_len = 0.05f;
    o5.nu = 0.f;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == 0, "nu = 0 runs");
    expect(same_bits(out.data(), ref.data(), (size_t)B * NQ) && same_bits(d.data(), dref.data(), (size_t)B), "nu 0 is the 72-byte call");
    expect(same_bits(nan_scale.data(), nan_copy.data(), nan_scale.size()), "scales nobody reads are not written");
    // 7. refusals write nothing
    o5.nu = 0.02f;
    sg = sg0;
    o.bone_scale = sg.data();
    root = root0;
    std::fill(out.begin(), out.end(), 7.0f);
    std::fill(energy.begin(), energy.end(), 7.0f);
    o.len_flags = 2;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "len_flags"), "an unknown flag is refused");
    o.len_flags = 0;
    o.reserved3 = 1;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "reserved3"), "reserved3 != 0 is refused");
    o.reserved3 = 0;
    o.nu_len = -1.f;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "nu_len"), "a negative nu_len is refused");
    o.nu_len = 0.05f;
    o.len_min = 0.f;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "len_min"), "half a clamp is refused");
    o.len_min = 0.5f;
    o.bone_scale = nullptr;
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "bone_scale"), "free scales that are NULL are refused");
    o.bone_scale = out.data();
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "bone_scale"), "scales in q_out are refused");
    o.bone_scale = root.data();
    expect(pndf_project_ex_cpu(h, q.data(), out.data(), d.data(), B, STEPS, opt) == PNDF_ERR_BAD_ARG && strstr(pndf_cpu_last_error(h), "bone_scale"), "scales in the root are refused");
    for (float x : out) expect(x == 7.0f, "a refused call writes nothing");
    for (float x : energy) expect(x == 7.0f, "a refused call writes no energy");
    expect(same_bits(root.data(), root0.data(), root.size()) && same_bits(sg.data(), sg0.data(), sg.size()), "a refused call writes no root and no scale");
    pndf_cpu_destroy(h);
    if (failures) {
        printf("skeleton_length_check: %d FAILURES\n", failures);
        return 1;
    }
    printf("skeleton_length_check: ok -- hand (15 joints), %d keypoints, %d scales: %d tracks of %d frames with one row of scales per track and per frame, no tracks, "
           "a track of %d frames (two blocks of the sum), %d steps, a joint mask, the anchor, confidences with NaN targets, free end frames, a free root, rates "
           "with zeros and a clamp: in place without tracks, the 168-byte call bit for bit with NULL scales and with unwritten ones, the 72-byte call with NaN "
           "scales that are not read, 7 refusals\n", K, S, P, T, LONG_T, STEPS);
    return 0;
}
