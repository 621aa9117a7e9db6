// Validation of pndf_project_options (include/posendf_amd.h), shared by pndf_project_ex (pndf_capi.hip) and its host twin
// pndf_project_ex_cpu (pndf_cpu.cpp): the two refuse the same structs with the same text.  And of pndf_project_options2, the options with
// a joint mask, which pndf_skel_project (pndf_skeleton.hip) and pndf_project_ex_cpu take besides, and of pndf_project_options3, the
// options with tracks (pose interpolation inside the step), and of pndf_project_options4, the options with an observation (motion
// denoising inside the step), and of pndf_project_options5, the options with 3D keypoints (keypoint fitting inside the step), and of
// pndf_project_options6, the options with a camera and a root (image fitting inside the step), which the same two take.
#pragma once
#include <math.h>

#include "../../include/posendf_amd.h"
#include "pndf_args.h"

// null = the defaults.  Returns nullptr and fills `out`, or the reason the struct is refused.
inline const char* pndf_check_project_options(const pndf_project_options* opt, pndf_project_options& out) {
    out.struct_size = (uint32_t)sizeof(pndf_project_options);
    out.step_size = 1.0f;
    out.renorm = PNDF_RENORM_NONE;
    out.tol = 0.0f;
    if (!opt) return nullptr;
    if (opt->struct_size != sizeof(pndf_project_options))
        return "pndf_project_options.struct_size is not sizeof(pndf_project_options): fill the struct with pndf_default_project_options";
    if (!isfinite(opt->step_size) || !(opt->step_size > 0.0f)) return "pndf_project_options.step_size must be finite and positive";
    if (!(opt->tol >= 0.0f)) return "pndf_project_options.tol must be zero or positive (and not NaN)";
    if (opt->renorm != PNDF_RENORM_NONE && opt->renorm != PNDF_RENORM_UNIT && opt->renorm != PNDF_RENORM_UNIT_FLIP)
        return "pndf_project_options.renorm is not a pndf_renorm mode";
    out = *opt;
    return nullptr;
}

// The checker of the two entry points that also take a pndf_project_options2 (pndf_skel_project, pndf_project_ex_cpu): struct_size
// says which of the two structs `opt` points to.  Returns nullptr, fills `out` from the struct (or its `base`) and sets `observed` to
// the mask (null: no joint is held), or the reason the struct is refused; nothing the mask points to is read here.
inline const char* pndf_check_project_options2(const pndf_project_options* opt, pndf_project_options& out, const uint32_t*& observed) {
    observed = nullptr;
    if (!opt || opt->struct_size == sizeof(pndf_project_options)) return pndf_check_project_options(opt, out);
    if (opt->struct_size != sizeof(pndf_project_options2)) {
        (void)pndf_check_project_options(nullptr, out);
        return "pndf_project_options.struct_size is neither sizeof(pndf_project_options) nor sizeof(pndf_project_options2): fill the "
               "struct with pndf_default_project_options";
    }
    const pndf_project_options2* o2 = (const pndf_project_options2*)opt;
    pndf_project_options base = o2->base;
    base.struct_size = (uint32_t)sizeof(pndf_project_options);
    if (const char* why = pndf_check_project_options(&base, out)) return why;
    if (o2->reserved != 0) return "pndf_project_options2.reserved must be 0";
    if ((uintptr_t)o2->observed & 3) return "pndf_project_options2.observed must be 4-byte aligned";
    observed = o2->observed;
    return nullptr;
}

// the longest track: the poses of one chunk of the skeleton unit (SK_CHUNK of pndf_skeleton.hip), so a track never straddles a seam
constexpr int32_t PNDF_TRACK_MAX_FRAMES = 16384;

// The tracks of a pndf_project_options3, validated: frames 0 = none (then lambda 0 and PNDF_TRACK_GIVEN)
struct PndfTracks {
    int32_t frames = 0;
    float lambda = 0.f;
    int32_t fill = PNDF_TRACK_GIVEN;
};

// The checker of the same two entry points for all three structs: a pndf_project_options3 brings the tracks of B poses besides.
// Returns nullptr and fills `out`, `observed` and `tracks`, or the reason the struct is refused.  That q_out does not overlap q_in
// when there are tracks is the caller's to check: it knows the size of a pose.
inline const char* pndf_check_project_options3(const pndf_project_options* opt, int64_t B, pndf_project_options& out,
                                               const uint32_t*& observed, PndfTracks& tracks) {
    tracks = PndfTracks();
    if (!opt || opt->struct_size != sizeof(pndf_project_options3)) {
        const char* why = pndf_check_project_options2(opt, out, observed);
        if (why && opt && opt->struct_size != sizeof(pndf_project_options) && opt->struct_size != sizeof(pndf_project_options2))
            return "pndf_project_options.struct_size is none of sizeof(pndf_project_options), sizeof(pndf_project_options2) and "
                   "sizeof(pndf_project_options3): fill the struct with pndf_default_project_options";
        return why;
    }
    const pndf_project_options3* o3 = (const pndf_project_options3*)opt;
    pndf_project_options2 base2 = o3->base2;
    base2.base.struct_size = (uint32_t)sizeof(pndf_project_options2);
    if (const char* why = pndf_check_project_options2(&base2.base, out, observed)) return why;
    observed = nullptr;      // (set again below: a refusal leaves no mask behind)
    if (o3->reserved2 != 0) return "pndf_project_options3.reserved2 must be 0";
    if (o3->fill != PNDF_TRACK_GIVEN && o3->fill != PNDF_TRACK_SLERP && o3->fill != PNDF_TRACK_NLERP)
        return "pndf_project_options3.fill is not a PNDF_TRACK_* mode";
    if (!(o3->lambda >= 0.f && o3->lambda <= 1.f)) return "pndf_project_options3.lambda must lie in [0, 1] (and not be NaN)";
    if (o3->frames == 0) {
        if (o3->lambda != 0.f) return "pndf_project_options3.lambda must be 0 when frames is 0 (no tracks)";
        if (o3->fill != PNDF_TRACK_GIVEN) return "pndf_project_options3.fill must be PNDF_TRACK_GIVEN when frames is 0 (no tracks)";
    } else {
        if (o3->frames < 2 || o3->frames > PNDF_TRACK_MAX_FRAMES) return "pndf_project_options3.frames must be 0 (no tracks) or 2 .. 16384";
        if (B > 0 && B % o3->frames != 0) return "pndf_project_options3.frames does not divide B: the poses are B / frames whole tracks";
    }
    observed = base2.observed;
    tracks.frames = o3->frames;
    tracks.lambda = o3->lambda;
    tracks.fill = o3->fill;
    return nullptr;
}

// The observation of a pndf_project_options4, validated: anchor null = no data term (then conf null and mu 0; a struct with mu == 0
// arrives here like that too, so its anchors are never read)
struct PndfData {
    const float* anchor = nullptr;
    const float* conf = nullptr;
    float mu = 0.f;
    bool free_ends = false;
    // whether a call needs the denoising form of the step at all: without either it is the call of the 48-byte struct
    bool any() const { return anchor || free_ends; }
};

// The checker of the same two entry points for all four structs: a pndf_project_options4 brings the observation of motion denoising
// besides.  Returns nullptr and fills `out`, `observed`, `tracks` and `data`, or the reason the struct is refused.  That anchor and
// conf do not overlap q_out is the caller's to check: it knows the size of a pose.
inline const char* pndf_check_project_options4(const pndf_project_options* opt, int64_t B, pndf_project_options& out,
                                               const uint32_t*& observed, PndfTracks& tracks, PndfData& data) {
    data = PndfData();
    if (!opt || opt->struct_size != sizeof(pndf_project_options4)) {
        const char* why = pndf_check_project_options3(opt, B, out, observed, tracks);
        if (why && opt && opt->struct_size != sizeof(pndf_project_options) && opt->struct_size != sizeof(pndf_project_options2) &&
            opt->struct_size != sizeof(pndf_project_options3))
            return "pndf_project_options.struct_size is none of sizeof(pndf_project_options), sizeof(pndf_project_options2), "
                   "sizeof(pndf_project_options3) and sizeof(pndf_project_options4): fill the struct with pndf_default_project_options";
        return why;
    }
    const pndf_project_options4* o4 = (const pndf_project_options4*)opt;
    pndf_project_options3 base3 = o4->base3;
    base3.base2.base.struct_size = (uint32_t)sizeof(pndf_project_options3);
    if (const char* why = pndf_check_project_options3(&base3.base2.base, B, out, observed, tracks)) return why;
    const uint32_t* mask = observed;
    const PndfTracks tr = tracks;
    observed = nullptr;      // (set again below: a refusal leaves no mask and no tracks behind)
    tracks = PndfTracks();
    if (!(o4->mu >= 0.f && o4->mu <= 1.f)) return "pndf_project_options4.mu must lie in [0, 1] (and not be NaN)";
    if (o4->flags & ~(uint32_t)PNDF_TRACK_FREE_ENDS) return "pndf_project_options4.flags has a bit other than PNDF_TRACK_FREE_ENDS";
    if (!o4->anchor && o4->mu != 0.f) return "pndf_project_options4.mu must be 0 when anchor is NULL (no data term)";
    if (!o4->anchor && o4->conf) return "pndf_project_options4.conf must be NULL when anchor is NULL (no data term)";
    if ((uintptr_t)o4->anchor & 3) return "pndf_project_options4.anchor must be 4-byte aligned";
    if ((uintptr_t)o4->conf & 3) return "pndf_project_options4.conf must be 4-byte aligned";
    if (o4->flags & PNDF_TRACK_FREE_ENDS) {
        if (tr.frames == 0) return "pndf_project_options4.flags: PNDF_TRACK_FREE_ENDS needs tracks (pndf_project_options3.frames >= 2)";
        if (tr.fill != PNDF_TRACK_GIVEN)
            return "pndf_project_options4.flags: PNDF_TRACK_FREE_ENDS needs pndf_project_options3.fill == PNDF_TRACK_GIVEN (a fill reads "
                   "only the end frames)";
    }
    observed = mask;
    tracks = tr;
    if (o4->mu != 0.f) {
        data.anchor = o4->anchor;
        data.conf = o4->conf;
        data.mu = o4->mu;
    }
    data.free_ends = (o4->flags & PNDF_TRACK_FREE_ENDS) != 0;
    return nullptr;
}

// What the entry point adds to the checker, knowing the size of a pose: every step reads the observation, so neither anchor [B,J,4]
// nor conf [B,J] may share memory with q_out [B,J,4] (q_in may: the observation is usually the start).  nullptr, or the reason.
inline const char* pndf_check_observation_apart(const PndfData& data, const float* q_out, int64_t B, int nj) {
    if (B <= 0 || !q_out) return nullptr;
    const uintptr_t o0 = (uintptr_t)q_out, o1 = (uintptr_t)(q_out + B * nj * 4);
    if (data.anchor && (uintptr_t)data.anchor < o1 && o0 < (uintptr_t)(data.anchor + B * nj * 4))
        return "pndf_project_options4.anchor must not overlap q_out: every step reads the observation";
    if (data.conf && (uintptr_t)data.conf < o1 && o0 < (uintptr_t)(data.conf + B * nj))
        return "pndf_project_options4.conf must not overlap q_out: every step reads the confidences";
    return nullptr;
}

// The keypoints of a pndf_project_options5, validated: target null = no keypoint term (a struct with nu == 0 arrives here like that
// too, so none of its keypoint arrays is read); `energy` stays, and without a term it is zeroed
constexpr int32_t PNDF_MAX_KEYPOINTS = 64;
struct PndfKeypoints {
    const float* target = nullptr;
    const float* conf = nullptr;
    float* energy = nullptr;
    const float* rest = nullptr;
    const int32_t* joint = nullptr;       // null: keypoint k is joint k
    const float* offset = nullptr;        // null: zeros
    int32_t K = 0;
    float nu = 0.f;
    // what the struct names whether or not there is a term (nu == 0 leaves `target` null): pndf_check_keypoints_apart refuses their
    // overlap with q_out either way, as the header says, though nothing reads them without a term
    const float* named_target = nullptr;
    const float* named_conf = nullptr;
    int32_t named_K = 0;
    int32_t dims = 3;                     // floats per target: 2 with the PNDF_KP_IMAGE of a pndf_project_options6
    int32_t views = 1;                    // V of a pndf_project_options8: the targets are [B,V,K,dims], the confidences [B,V,K]
    bool any() const { return target != nullptr; }
};

// The checker of the same two entry points for all five structs: a pndf_project_options5 brings the 3D keypoints of a fit besides.
// `nj`: the joint count of the handle, which sizes the host tables rest [nj,3], kp_joint [K] and kp_offset [K,3]; they are read here
// (and only when there is a term: kp_target != NULL and nu != 0).  Returns nullptr and fills `out`, `observed`, `tracks`, `data` and
// `kp`, or the reason the struct is refused.  That the device arrays do not overlap q_out is the caller's to check.
inline const char* pndf_check_project_options5(const pndf_project_options* opt, int64_t B, int nj, pndf_project_options& out,
                                               const uint32_t*& observed, PndfTracks& tracks, PndfData& data, PndfKeypoints& kp) {
    kp = PndfKeypoints();
    if (!opt || opt->struct_size != sizeof(pndf_project_options5)) {
        const char* why = pndf_check_project_options4(opt, B, out, observed, tracks, data);
        if (why && opt && opt->struct_size != sizeof(pndf_project_options) && opt->struct_size != sizeof(pndf_project_options2) &&
            opt->struct_size != sizeof(pndf_project_options3) && opt->struct_size != sizeof(pndf_project_options4))
            return "pndf_project_options.struct_size is none of sizeof(pndf_project_options), sizeof(pndf_project_options2), "
                   "sizeof(pndf_project_options3), sizeof(pndf_project_options4) and sizeof(pndf_project_options5): fill the struct with "
                   "pndf_default_project_options";
        return why;
    }
    const pndf_project_options5* o5 = (const pndf_project_options5*)opt;
    pndf_project_options4 base4 = o5->base4;
    base4.base3.base2.base.struct_size = (uint32_t)sizeof(pndf_project_options4);
    if (const char* why = pndf_check_project_options4(&base4.base3.base2.base, B, out, observed, tracks, data)) return why;
    const uint32_t* mask = observed;
    const PndfTracks tr = tracks;
    const PndfData da = data;
    observed = nullptr;      // (set again below: a refusal leaves no mask, no tracks and no observation behind)
    tracks = PndfTracks();
    data = PndfData();
    if (!isfinite(o5->nu) || !(o5->nu >= 0.f)) return "pndf_project_options5.nu must be finite and zero or positive";
    if ((uintptr_t)o5->kp_target & 3) return "pndf_project_options5.kp_target must be 4-byte aligned";
    if ((uintptr_t)o5->kp_conf & 3) return "pndf_project_options5.kp_conf must be 4-byte aligned";
    if ((uintptr_t)o5->kp_energy & 3) return "pndf_project_options5.kp_energy must be 4-byte aligned";
    if ((uintptr_t)o5->rest & 3) return "pndf_project_options5.rest must be 4-byte aligned";
    if ((uintptr_t)o5->kp_joint & 3) return "pndf_project_options5.kp_joint must be 4-byte aligned";
    if ((uintptr_t)o5->kp_offset & 3) return "pndf_project_options5.kp_offset must be 4-byte aligned";
    if (o5->kp_target) {
        const int32_t K = o5->n_keypoints;
        if (K < 1 || K > PNDF_MAX_KEYPOINTS) return "pndf_project_options5.n_keypoints must lie in 1 .. 64 when kp_target is not NULL";
        if (!o5->rest) return "pndf_project_options5.rest must not be NULL when kp_target is not NULL: the rest offsets [J,3] of the joint tree";
        if (!o5->kp_joint && K != nj)
            return "pndf_project_options5.kp_joint is NULL (keypoint k is joint k), so n_keypoints must equal the joint count";
        kp.named_target = o5->kp_target;
        kp.named_conf = o5->kp_conf;
        kp.named_K = K;
        if (o5->nu != 0.f) {      // the tables are read only when there is a term
            if (o5->kp_joint)
                for (int32_t k = 0; k < K; ++k)
                    if (o5->kp_joint[k] < 0 || o5->kp_joint[k] >= nj) return "pndf_project_options5.kp_joint has an entry outside 0 .. J-1";
            for (int i = 0; i < 3 * nj; ++i)
                if (!isfinite(o5->rest[i])) return "pndf_project_options5.rest has a value that is not finite";
            if (o5->kp_offset)
                for (int32_t i = 0; i < 3 * K; ++i)
                    if (!isfinite(o5->kp_offset[i])) return "pndf_project_options5.kp_offset has a value that is not finite";
            kp.target = o5->kp_target;
            kp.conf = o5->kp_conf;
            kp.rest = o5->rest;
            kp.joint = o5->kp_joint;
            kp.offset = o5->kp_offset;
            kp.K = K;
            kp.nu = o5->nu;
        }
    }
    kp.energy = o5->kp_energy;
    observed = mask;
    tracks = tr;
    data = da;
    return nullptr;
}

// What the entry point adds to that checker, knowing B: every step reads the targets and the confidences and the last one writes the
// energies, so none of kp_target [B,K,3], kp_conf [B,K] and kp_energy [B] may share memory with q_out [B,J,4].  nullptr, or the reason.
// The arrays are compared as the struct names them, with a term (nu != 0) or without.
inline const char* pndf_check_keypoints_apart(const PndfKeypoints& kp, const float* q_out, int64_t B, int nj) {
    if (B <= 0 || !q_out) return nullptr;
    const uintptr_t o0 = (uintptr_t)q_out, o1 = (uintptr_t)(q_out + B * nj * 4);
    if (kp.named_target && (uintptr_t)kp.named_target < o1 && o0 < (uintptr_t)(kp.named_target + B * kp.views * kp.named_K * kp.dims))
        return "pndf_project_options5.kp_target must not overlap q_out: every step reads the targets";
    if (kp.named_conf && (uintptr_t)kp.named_conf < o1 && o0 < (uintptr_t)(kp.named_conf + B * kp.views * kp.named_K))
        return "pndf_project_options5.kp_conf must not overlap q_out: every step reads the confidences";
    if (kp.energy && (uintptr_t)kp.energy < o1 && o0 < (uintptr_t)(kp.energy + B))
        return "pndf_project_options5.kp_energy must not overlap q_out";
    return nullptr;
}

// The camera and the root of a pndf_project_options6, validated: without a keypoint term (kp_target NULL or nu == 0) there is no energy
// for the root to descend, `root` stays null and nothing of it is read or written, whatever its weights; `named_root` is what the struct
// names either way (pndf_check_root_apart refuses its overlap with q_out as the header says)
struct PndfCameraTerm {
    float* root = nullptr;      // null: identity, C_k = P_k without arithmetic
    float* named_root = nullptr;
    float fx = 1.f, fy = 1.f, cx = 0.f, cy = 0.f, rho = 0.f;
    float nu_rot = 0.f, nu_trans = 0.f;
    bool image = false;
    bool moves() const { return root && (nu_rot > 0.f || nu_trans > 0.f); }
    // whether a call needs the camera form of the fitting step at all: without either it is the call of the 128-byte struct
    bool any() const { return root || image; }
};

// The checker of the same two entry points for all six structs: a pndf_project_options6 brings the camera and the root of a fit to 2D
// keypoints besides.  Returns nullptr and fills `out`, `observed`, `tracks`, `data`, `kp` and `cam`, or the reason the struct is refused.
// That root does not overlap the other arrays is the caller's to check (pndf_check_root_apart).
inline const char* pndf_check_project_options6(const pndf_project_options* opt, int64_t B, int nj, pndf_project_options& out,
                                               const uint32_t*& observed, PndfTracks& tracks, PndfData& data, PndfKeypoints& kp,
                                               PndfCameraTerm& cam) {
    cam = PndfCameraTerm();
    if (!opt || opt->struct_size != sizeof(pndf_project_options6)) {
        const char* why = pndf_check_project_options5(opt, B, nj, out, observed, tracks, data, kp);
        if (why && opt && opt->struct_size != sizeof(pndf_project_options) && opt->struct_size != sizeof(pndf_project_options2) &&
            opt->struct_size != sizeof(pndf_project_options3) && opt->struct_size != sizeof(pndf_project_options4) &&
            opt->struct_size != sizeof(pndf_project_options5))
            return "pndf_project_options.struct_size is none of sizeof(pndf_project_options), sizeof(pndf_project_options2), "
                   "sizeof(pndf_project_options3), sizeof(pndf_project_options4), sizeof(pndf_project_options5) and "
                   "sizeof(pndf_project_options6): fill the struct with pndf_default_project_options";
        return why;
    }
    const pndf_project_options6* o6 = (const pndf_project_options6*)opt;
    pndf_project_options5 base5 = o6->base5;
    base5.base4.base3.base2.base.struct_size = (uint32_t)sizeof(pndf_project_options5);
    if (const char* why = pndf_check_project_options5(&base5.base4.base3.base2.base, B, nj, out, observed, tracks, data, kp)) return why;
    const uint32_t* mask = observed;
    const PndfTracks tr = tracks;
    const PndfData da = data;
    const PndfKeypoints k5 = kp;
    observed = nullptr;      // (set again below: a refusal leaves nothing behind)
    tracks = PndfTracks();
    data = PndfData();
    kp = PndfKeypoints();
    if (o6->kp_flags & ~(uint32_t)PNDF_KP_IMAGE) return "pndf_project_options6.kp_flags has a bit other than PNDF_KP_IMAGE";
    const bool image = (o6->kp_flags & PNDF_KP_IMAGE) != 0;
    if (!isfinite(o6->rho) || !(o6->rho >= 0.f)) return "pndf_project_options6.rho must be finite and zero or positive";
    if (!isfinite(o6->nu_rot) || !(o6->nu_rot >= 0.f)) return "pndf_project_options6.nu_rot must be finite and zero or positive";
    if (!isfinite(o6->nu_trans) || !(o6->nu_trans >= 0.f)) return "pndf_project_options6.nu_trans must be finite and zero or positive";
    if (o6->rho != 0.f && !image) return "pndf_project_options6.rho must be 0 without PNDF_KP_IMAGE: it is the robustifier of the image residual";
    if (image) {
        if (!isfinite(o6->fx) || !(o6->fx > 0.f)) return "pndf_project_options6.fx must be finite and positive with PNDF_KP_IMAGE";
        if (!isfinite(o6->fy) || !(o6->fy > 0.f)) return "pndf_project_options6.fy must be finite and positive with PNDF_KP_IMAGE";
        if (!isfinite(o6->cx)) return "pndf_project_options6.cx must be finite with PNDF_KP_IMAGE";
        if (!isfinite(o6->cy)) return "pndf_project_options6.cy must be finite with PNDF_KP_IMAGE";
    }
    if (!o6->root && (o6->nu_rot > 0.f || o6->nu_trans > 0.f))
        return "pndf_project_options6.root must not be NULL when nu_rot or nu_trans is positive";
    if ((uintptr_t)o6->root & 3) return "pndf_project_options6.root must be 4-byte aligned";
    observed = mask;
    tracks = tr;
    data = da;
    kp = k5;
    cam.named_root = o6->root;
    cam.nu_rot = o6->nu_rot;
    cam.nu_trans = o6->nu_trans;
    if (image) kp.dims = 2;
    if (kp.any()) {
        cam.root = o6->root;
        cam.image = image;
        cam.rho = o6->rho;
        if (image) { cam.fx = o6->fx; cam.fy = o6->fy; cam.cx = o6->cx; cam.cy = o6->cy; }
    }
    return nullptr;
}

// What the entry point adds to that checker, knowing B and the poses: root [B,7] is read by every step, so it may not share memory with
// q_out [B,J,4]; and it is written by every step when a root weight is positive, so then it may not share memory with anything the
// steps read or the call writes: q_in, anchor, conf, kp_target, kp_conf, kp_energy.  nullptr, or the reason.  The keypoint arrays are
// compared as the struct names them, the observation as it is read (none with mu == 0).
inline const char* pndf_check_root_apart(const PndfCameraTerm& cam, const PndfData& data, const PndfKeypoints& kp, const float* q_in,
                                         const float* q_out, int64_t B, int nj) {
    if (B <= 0 || !cam.named_root) return nullptr;
    const uintptr_t r0 = (uintptr_t)cam.named_root, r1 = (uintptr_t)(cam.named_root + B * 7);
    auto meets = [&](const float* p, int64_t floats) { return p && (uintptr_t)p < r1 && r0 < (uintptr_t)(p + floats); };
    if (meets(q_out, B * nj * 4)) return "pndf_project_options6.root must not overlap q_out: every step reads the root";
    if (!(cam.nu_rot > 0.f || cam.nu_trans > 0.f)) return nullptr;
    if (meets(q_in, B * nj * 4)) return "pndf_project_options6.root must not overlap q_in when nu_rot or nu_trans is positive: every step writes the root";
    if (meets(data.anchor, B * nj * 4)) return "pndf_project_options6.root must not overlap pndf_project_options4.anchor when nu_rot or nu_trans is positive";
    if (meets(data.conf, (int64_t)B * nj)) return "pndf_project_options6.root must not overlap pndf_project_options4.conf when nu_rot or nu_trans is positive";
    if (meets(kp.named_target, B * kp.views * kp.named_K * kp.dims)) return "pndf_project_options6.root must not overlap kp_target when nu_rot or nu_trans is positive";
    if (meets(kp.named_conf, (int64_t)B * kp.views * kp.named_K)) return "pndf_project_options6.root must not overlap kp_conf when nu_rot or nu_trans is positive";
    if (meets(kp.energy, B)) return "pndf_project_options6.root must not overlap kp_energy when nu_rot or nu_trans is positive";
    return nullptr;
}

// The bone lengths of a pndf_project_options7, validated: without a keypoint term (kp_target NULL or nu == 0) `scale` stays null and
// nothing of it is read or written; `named_scale` is what the struct names either way (pndf_check_lengths_apart refuses its overlaps).
// S = J + K scales per row; G rows: one per track of `frames` frames, or one per pose.
constexpr int32_t PNDF_MAX_SCALES = 96;      // 32 joints + 64 keypoints
struct PndfLengths {
    float* scale = nullptr;
    float* named_scale = nullptr;
    int64_t named_floats = 0;      // G * S of the struct as it names its keypoints
    int32_t S = 0;
    int32_t group = 1;             // frames per group: T, or 1
    float nu_len = 0.f, kappa = 0.f, len_min = 0.f, len_max = 0.f;
    float rate[PNDF_MAX_SCALES];
    bool any() const { return scale != nullptr; }
    bool moves() const { return scale && nu_len > 0.f; }
};

// The checker of the same two entry points for all seven structs: a pndf_project_options7 brings the bone lengths besides.  Returns nullptr
// and fills `out`, `observed`, `tracks`, `data`, `kp`, `cam` and `len`, or the reason the struct is refused.  That bone_scale does not
// overlap the other arrays is the caller's to check (pndf_check_lengths_apart).  PNDF_LEN_PER_POSE with frames == 0 is accepted: there
// every pose is its own group anyway.
inline const char* pndf_check_project_options7(const pndf_project_options* opt, int64_t B, int nj, pndf_project_options& out,
                                               const uint32_t*& observed, PndfTracks& tracks, PndfData& data, PndfKeypoints& kp,
                                               PndfCameraTerm& cam, PndfLengths& len) {
    len = PndfLengths();
    for (int i = 0; i < PNDF_MAX_SCALES; ++i) len.rate[i] = 1.0f;
    if (!opt || opt->struct_size != sizeof(pndf_project_options7)) {
        const char* why = pndf_check_project_options6(opt, B, nj, out, observed, tracks, data, kp, cam);
        if (why && opt && opt->struct_size != sizeof(pndf_project_options) && opt->struct_size != sizeof(pndf_project_options2) &&
            opt->struct_size != sizeof(pndf_project_options3) && opt->struct_size != sizeof(pndf_project_options4) &&
            opt->struct_size != sizeof(pndf_project_options5) && opt->struct_size != sizeof(pndf_project_options6))
            return "pndf_project_options.struct_size is none of sizeof(pndf_project_options), sizeof(pndf_project_options2), "
                   "sizeof(pndf_project_options3), sizeof(pndf_project_options4), sizeof(pndf_project_options5), "
                   "sizeof(pndf_project_options6) and sizeof(pndf_project_options7): fill the struct with pndf_default_project_options";
        return why;
    }
    const pndf_project_options7* o7 = (const pndf_project_options7*)opt;
    pndf_project_options6 base6 = o7->base6;
    base6.base5.base4.base3.base2.base.struct_size = (uint32_t)sizeof(pndf_project_options6);
    if (const char* why = pndf_check_project_options6(&base6.base5.base4.base3.base2.base, B, nj, out, observed, tracks, data, kp, cam)) return why;
    const uint32_t* mask = observed;
    const PndfTracks tr = tracks;
    const PndfData da = data;
    const PndfKeypoints k6 = kp;
    const PndfCameraTerm c6 = cam;
    observed = nullptr;      // (set again below: a refusal leaves nothing behind)
    tracks = PndfTracks();
    data = PndfData();
    kp = PndfKeypoints();
    cam = PndfCameraTerm();
    if (o7->reserved3 != 0u) return "pndf_project_options7.reserved3 must be 0";
    if (o7->len_flags & ~(uint32_t)PNDF_LEN_PER_POSE) return "pndf_project_options7.len_flags has a bit other than PNDF_LEN_PER_POSE";
    if (!isfinite(o7->nu_len) || !(o7->nu_len >= 0.f)) return "pndf_project_options7.nu_len must be finite and zero or positive";
    if (!isfinite(o7->kappa) || !(o7->kappa >= 0.f)) return "pndf_project_options7.kappa must be finite and zero or positive";
    if (!(o7->len_min == 0.f && o7->len_max == 0.f)) {
        if (!isfinite(o7->len_min) || !(o7->len_min > 0.f))
            return "pndf_project_options7.len_min must be finite and positive when a clamp is given (len_min and len_max both 0: none)";
        if (!isfinite(o7->len_max) || !(o7->len_max >= o7->len_min))
            return "pndf_project_options7.len_max must be finite and not below len_min when a clamp is given";
    }
    if ((uintptr_t)o7->len_rate & 3) return "pndf_project_options7.len_rate must be 4-byte aligned";
    if ((uintptr_t)o7->bone_scale & 3) return "pndf_project_options7.bone_scale must be 4-byte aligned";
    if (!o7->bone_scale && o7->nu_len > 0.f) return "pndf_project_options7.bone_scale must not be NULL when nu_len is positive";
    const int32_t S = nj + k6.named_K;      // without kp_target there are no keypoints and no term: len_rate is not read
    if (o7->len_rate && k6.named_target)
        for (int32_t i = 0; i < S; ++i)
            if (!isfinite(o7->len_rate[i]) || !(o7->len_rate[i] >= 0.f))
                return "pndf_project_options7.len_rate has an entry that is negative or not finite";
    observed = mask;
    tracks = tr;
    data = da;
    kp = k6;
    cam = c6;
    const bool per_pose = (o7->len_flags & PNDF_LEN_PER_POSE) != 0 || tr.frames < 2;
    len.S = S;
    len.group = per_pose ? 1 : tr.frames;
    len.named_scale = o7->bone_scale;
    len.named_floats = (B > 0 ? B / len.group : 0) * (int64_t)S;
    len.nu_len = o7->nu_len;
    len.kappa = o7->kappa;
    len.len_min = o7->len_min;
    len.len_max = o7->len_max;
    if (o7->len_rate && k6.named_target)
        for (int32_t i = 0; i < S; ++i) len.rate[i] = o7->len_rate[i];
    if (kp.any()) len.scale = o7->bone_scale;
    return nullptr;
}

// What the entry point adds to that checker, knowing B and the poses: bone_scale [G,S] is read by every step and written by every step
// with nu_len > 0, so it may share memory with nothing the steps read or the call writes: q_out, q_in, root, anchor, conf, kp_target,
// kp_conf, kp_energy.  nullptr, or the reason.  The arrays are compared as the struct names them.
inline const char* pndf_check_lengths_apart(const PndfLengths& len, const PndfCameraTerm& cam, const PndfData& data, const PndfKeypoints& kp,
                                            const float* q_in, const float* q_out, int64_t B, int nj) {
    if (B <= 0 || !len.named_scale) return nullptr;
    const uintptr_t r0 = (uintptr_t)len.named_scale, r1 = (uintptr_t)(len.named_scale + len.named_floats);
    auto meets = [&](const float* p, int64_t floats) { return p && (uintptr_t)p < r1 && r0 < (uintptr_t)(p + floats); };
    if (meets(q_out, B * nj * 4)) return "pndf_project_options7.bone_scale must not overlap q_out";
    if (meets(q_in, B * nj * 4)) return "pndf_project_options7.bone_scale must not overlap q_in";
    if (meets(cam.named_root, B * 7)) return "pndf_project_options7.bone_scale must not overlap pndf_project_options6.root";
    if (meets(data.anchor, B * nj * 4)) return "pndf_project_options7.bone_scale must not overlap pndf_project_options4.anchor";
    if (meets(data.conf, (int64_t)B * nj)) return "pndf_project_options7.bone_scale must not overlap pndf_project_options4.conf";
    if (meets(kp.named_target, B * kp.views * kp.named_K * kp.dims)) return "pndf_project_options7.bone_scale must not overlap kp_target";
    if (meets(kp.named_conf, (int64_t)B * kp.views * kp.named_K)) return "pndf_project_options7.bone_scale must not overlap kp_conf";
    if (meets(kp.energy, B)) return "pndf_project_options7.bone_scale must not overlap kp_energy";
    return nullptr;
}

// The views of a pndf_project_options8, validated and copied (the table is host memory that is read during the call only): without a
// keypoint term (nu == 0) V stays 0 and the call is the one without views.
struct PndfViews {
    int32_t V = 0;
    float table[PNDF_FK_MAX_VIEWS * 16];      // row v: fx, fy, cx, cy, R_v [9] row-major, t_v [3]
    bool any() const { return V > 0; }
};

// The checker of the same two entry points for all eight structs: a pndf_project_options8 brings the views besides.  Returns nullptr and
// fills `out`, `observed`, `tracks`, `data`, `kp` (with the views' count in kp.views, which sizes kp_target and kp_conf in the overlap
// checks that follow), `cam`, `len` and `vw`, or the reason the struct is refused.
inline const char* pndf_check_project_options8(const pndf_project_options* opt, int64_t B, int nj, pndf_project_options& out,
                                               const uint32_t*& observed, PndfTracks& tracks, PndfData& data, PndfKeypoints& kp,
                                               PndfCameraTerm& cam, PndfLengths& len, PndfViews& vw) {
    vw.V = 0;
    for (int i = 0; i < PNDF_FK_MAX_VIEWS * 16; ++i) vw.table[i] = 0.f;
    if (!opt || opt->struct_size != sizeof(pndf_project_options8)) {
        const char* why = pndf_check_project_options7(opt, B, nj, out, observed, tracks, data, kp, cam, len);
        if (why && opt && opt->struct_size != sizeof(pndf_project_options) && opt->struct_size != sizeof(pndf_project_options2) &&
            opt->struct_size != sizeof(pndf_project_options3) && opt->struct_size != sizeof(pndf_project_options4) &&
            opt->struct_size != sizeof(pndf_project_options5) && opt->struct_size != sizeof(pndf_project_options6) &&
            opt->struct_size != sizeof(pndf_project_options7))
            return "pndf_project_options.struct_size is none of sizeof(pndf_project_options), sizeof(pndf_project_options2), "
                   "sizeof(pndf_project_options3), sizeof(pndf_project_options4), sizeof(pndf_project_options5), "
                   "sizeof(pndf_project_options6), sizeof(pndf_project_options7) and sizeof(pndf_project_options8): fill the struct with "
                   "pndf_default_project_options";
        return why;
    }
    const pndf_project_options8* o8 = (const pndf_project_options8*)opt;
    // what the struct says of itself first: a refusal here has filled nothing
    out = pndf_project_options();
    observed = nullptr;
    tracks = PndfTracks();
    data = PndfData();
    kp = PndfKeypoints();
    cam = PndfCameraTerm();
    if (o8->reserved4 != 0u) return "pndf_project_options8.reserved4 must be 0";
    if (o8->n_views < 0 || o8->n_views > PNDF_FK_MAX_VIEWS) return "pndf_project_options8.n_views must lie in 0 .. 8";
    if ((uintptr_t)o8->views & 3) return "pndf_project_options8.views must be 4-byte aligned";
    if (!o8->views && o8->n_views != 0) return "pndf_project_options8.views must not be NULL when n_views is positive";
    if (o8->views && o8->n_views == 0) return "pndf_project_options8.n_views must be positive when views is not NULL";
    if (o8->n_views > 0) {
        if (!(o8->base7.base6.kp_flags & PNDF_KP_IMAGE)) return "pndf_project_options8.n_views is positive, so pndf_project_options6.kp_flags must have PNDF_KP_IMAGE";
        if (!o8->base7.base6.base5.kp_target) return "pndf_project_options8.n_views is positive, so pndf_project_options5.kp_target must not be NULL";
        for (int32_t v = 0; v < o8->n_views; ++v) {
            const float* r = o8->views + 16 * v;
            if (!isfinite(r[0]) || !(r[0] > 0.f)) return "pndf_project_options8.views has a view whose fx is not finite and positive";
            if (!isfinite(r[1]) || !(r[1] > 0.f)) return "pndf_project_options8.views has a view whose fy is not finite and positive";
            for (int i = 2; i < 16; ++i)
                if (!isfinite(r[i])) return "pndf_project_options8.views has an entry that is not finite";
        }
    }
    pndf_project_options7 base7 = o8->base7;
    base7.base6.base5.base4.base3.base2.base.struct_size = (uint32_t)sizeof(pndf_project_options7);
    if (o8->n_views > 0) {      // the intrinsics of base6 are not read: whatever they hold is not refused
        base7.base6.fx = base7.base6.fy = 1.f;
        base7.base6.cx = base7.base6.cy = 0.f;
    }
    if (const char* why = pndf_check_project_options7(&base7.base6.base5.base4.base3.base2.base, B, nj, out, observed, tracks, data, kp, cam, len)) return why;
    if (o8->n_views > 0) {
        kp.views = o8->n_views;
        if (kp.any()) {
            vw.V = o8->n_views;
            for (int i = 0; i < 16 * o8->n_views; ++i) vw.table[i] = o8->views[i];
        }
    }
    return nullptr;
}

// The root trajectory of a pndf_project_options9, validated: without a keypoint term (kp_target NULL or nu == 0) every weight stays 0 and
// nothing of the root or the anchor is read or written; `named_anchor` is what the struct names either way (pndf_check_root_anchor_apart
// refuses its overlaps).
struct PndfRootSmooth {
    const float* anchor = nullptr;      // [B,7], or null: no data term
    const float* named_anchor = nullptr;
    float lambda_rot = 0.f, lambda_trans = 0.f, mu_rot = 0.f, mu_trans = 0.f;
    // whether a call needs the coupled form of the root's step at all: without it it is the call of the 224-byte struct
    bool any() const { return lambda_rot > 0.f || lambda_trans > 0.f || mu_rot > 0.f || mu_trans > 0.f; }
};

// The checker of the same two entry points for all nine structs: a pndf_project_options9 brings the root's trajectory besides.  Returns
// nullptr and fills `out`, `observed`, `tracks`, `data`, `kp`, `cam`, `len`, `vw` and `rs`, or the reason the struct is refused.  That
// root_anchor does not overlap root or q_out is the caller's to check (pndf_check_root_anchor_apart).
inline const char* pndf_check_project_options9(const pndf_project_options* opt, int64_t B, int nj, pndf_project_options& out,
                                               const uint32_t*& observed, PndfTracks& tracks, PndfData& data, PndfKeypoints& kp,
                                               PndfCameraTerm& cam, PndfLengths& len, PndfViews& vw, PndfRootSmooth& rs) {
    rs = PndfRootSmooth();
    if (!opt || opt->struct_size != sizeof(pndf_project_options9)) {
        const char* why = pndf_check_project_options8(opt, B, nj, out, observed, tracks, data, kp, cam, len, vw);
        if (why && opt && opt->struct_size != sizeof(pndf_project_options) && opt->struct_size != sizeof(pndf_project_options2) &&
            opt->struct_size != sizeof(pndf_project_options3) && opt->struct_size != sizeof(pndf_project_options4) &&
            opt->struct_size != sizeof(pndf_project_options5) && opt->struct_size != sizeof(pndf_project_options6) &&
            opt->struct_size != sizeof(pndf_project_options7) && opt->struct_size != sizeof(pndf_project_options8))
            return "pndf_project_options.struct_size is none of sizeof(pndf_project_options), sizeof(pndf_project_options2), "
                   "sizeof(pndf_project_options3), sizeof(pndf_project_options4), sizeof(pndf_project_options5), "
                   "sizeof(pndf_project_options6), sizeof(pndf_project_options7), sizeof(pndf_project_options8) and "
                   "sizeof(pndf_project_options9): fill the struct with pndf_default_project_options";
        return why;
    }
    const pndf_project_options9* o9 = (const pndf_project_options9*)opt;
    // what the struct says of itself first: a refusal here has filled nothing
    out = pndf_project_options();
    observed = nullptr;
    tracks = PndfTracks();
    data = PndfData();
    kp = PndfKeypoints();
    cam = PndfCameraTerm();
    len = PndfLengths();
    for (int i = 0; i < PNDF_MAX_SCALES; ++i) len.rate[i] = 1.0f;
    vw.V = 0;
    auto unit = [](float v) { return v >= 0.f && v <= 1.f; };      // false for a NaN
    const pndf_project_options6& o6 = o9->base8.base7.base6;
    const bool rot = o9->lambda_rot > 0.f || o9->mu_rot > 0.f, trans = o9->lambda_trans > 0.f || o9->mu_trans > 0.f;
    if (o9->reserved5 != 0u) return "pndf_project_options9.reserved5 must be 0";
    if (!unit(o9->lambda_rot)) return "pndf_project_options9.lambda_rot must lie in [0, 1] (and not be NaN)";
    if (!unit(o9->lambda_trans)) return "pndf_project_options9.lambda_trans must lie in [0, 1] (and not be NaN)";
    if (!unit(o9->mu_rot)) return "pndf_project_options9.mu_rot must lie in [0, 1] (and not be NaN)";
    if (!unit(o9->mu_trans)) return "pndf_project_options9.mu_trans must lie in [0, 1] (and not be NaN)";
    if (o9->lambda_rot > 0.f && o6.base5.base4.base3.frames == 0)
        return "pndf_project_options9.lambda_rot must be 0 when pndf_project_options3.frames is 0 (no tracks)";
    if (o9->lambda_trans > 0.f && o6.base5.base4.base3.frames == 0)
        return "pndf_project_options9.lambda_trans must be 0 when pndf_project_options3.frames is 0 (no tracks)";
    // (a nu that is negative or not finite is base8's to refuse, below, with its own text)
    if (o9->lambda_rot > 0.f && o6.nu_rot == 0.f) return "pndf_project_options9.lambda_rot must be 0 when pndf_project_options6.nu_rot is 0: the rotation is held";
    if (o9->mu_rot > 0.f && o6.nu_rot == 0.f) return "pndf_project_options9.mu_rot must be 0 when pndf_project_options6.nu_rot is 0: the rotation is held";
    if (o9->lambda_trans > 0.f && o6.nu_trans == 0.f) return "pndf_project_options9.lambda_trans must be 0 when pndf_project_options6.nu_trans is 0: the translation is held";
    if (o9->mu_trans > 0.f && o6.nu_trans == 0.f) return "pndf_project_options9.mu_trans must be 0 when pndf_project_options6.nu_trans is 0: the translation is held";
    if ((rot || trans) && !o6.root) return "pndf_project_options6.root must not be NULL when a lambda or mu of pndf_project_options9 is positive";
    if ((o9->mu_rot > 0.f || o9->mu_trans > 0.f) && !o9->root_anchor)
        return "pndf_project_options9.root_anchor must not be NULL when mu_rot or mu_trans is positive";
    if (o9->root_anchor && !(o9->mu_rot > 0.f || o9->mu_trans > 0.f))
        return "pndf_project_options9.root_anchor must be NULL when mu_rot and mu_trans are 0 (no data term)";
    if ((uintptr_t)o9->root_anchor & 3) return "pndf_project_options9.root_anchor must be 4-byte aligned";
    pndf_project_options8 base8 = o9->base8;
    base8.base7.base6.base5.base4.base3.base2.base.struct_size = (uint32_t)sizeof(pndf_project_options8);
    if (const char* why = pndf_check_project_options8(&base8.base7.base6.base5.base4.base3.base2.base, B, nj, out, observed, tracks, data, kp, cam, len, vw)) return why;
    rs.named_anchor = o9->root_anchor;
    if (kp.any()) {
        rs.anchor = o9->root_anchor;
        rs.lambda_rot = o9->lambda_rot;
        rs.lambda_trans = o9->lambda_trans;
        rs.mu_rot = o9->mu_rot;
        rs.mu_trans = o9->mu_trans;
    }
    return nullptr;
}

// What the entry point adds to that checker, knowing B and the poses: every step reads root_anchor [B,7] and writes root and q_out, so it
// may share memory with neither.  nullptr, or the reason.  The arrays are compared as the struct names them.
inline const char* pndf_check_root_anchor_apart(const PndfRootSmooth& rs, const PndfCameraTerm& cam, const float* q_out, int64_t B, int nj) {
    if (B <= 0 || !rs.named_anchor) return nullptr;
    const uintptr_t r0 = (uintptr_t)rs.named_anchor, r1 = (uintptr_t)(rs.named_anchor + B * 7);
    auto meets = [&](const float* p, int64_t floats) { return p && (uintptr_t)p < r1 && r0 < (uintptr_t)(p + floats); };
    if (meets(cam.named_root, B * 7)) return "pndf_project_options9.root_anchor must not overlap pndf_project_options6.root: every step writes the root";
    if (meets(q_out, B * nj * 4)) return "pndf_project_options9.root_anchor must not overlap q_out";
    return nullptr;
}

// The moving cameras of a pndf_project_options10, validated as far as the host can: the table lives where the step runs (device memory
// for the skeleton unit), so its VALUES are not looked at here -- pndf_fk_cams_keypoint switches off a view whose focal lengths are not
// positive.  Without a keypoint term (kp_target NULL or nu == 0) `table` stays null and nothing of it is read; `named_table` is what the
// struct names either way (pndf_check_pose_views_apart refuses its overlaps).
struct PndfPoseViews {
    const float* table = nullptr;      // [B,V,16], or [frames,V,16] with per_frame; null: none
    const float* named_table = nullptr;
    int32_t V = 0;
    int32_t frames = 0;                // per_frame: T, pose c reads block c % T; else 0: pose c reads block c
    bool any() const { return table != nullptr; }
    // the block of pose number `pose` of the call
    const float* block(int64_t pose) const { return table + (frames ? pose % frames : pose) * ((int64_t)V * 16); }
};

// The checker of the same two entry points for all ten structs: a pndf_project_options10 brings the moving cameras besides.  Returns
// nullptr and fills `out`, `observed`, `tracks`, `data`, `kp` (with the views' count in kp.views, as a pndf_project_options8 does),
// `cam`, `len`, `vw`, `rs` and `pv`, or the reason the struct is refused.  That pose_views does not overlap what the steps write is the
// caller's to check (pndf_check_pose_views_apart).
inline const char* pndf_check_project_options10(const pndf_project_options* opt, int64_t B, int nj, pndf_project_options& out,
                                                const uint32_t*& observed, PndfTracks& tracks, PndfData& data, PndfKeypoints& kp,
                                                PndfCameraTerm& cam, PndfLengths& len, PndfViews& vw, PndfRootSmooth& rs,
                                                PndfPoseViews& pv) {
    pv = PndfPoseViews();
    if (!opt || opt->struct_size != sizeof(pndf_project_options10)) {
        const char* why = pndf_check_project_options9(opt, B, nj, out, observed, tracks, data, kp, cam, len, vw, rs);
        if (why && opt && opt->struct_size != sizeof(pndf_project_options) && opt->struct_size != sizeof(pndf_project_options2) &&
            opt->struct_size != sizeof(pndf_project_options3) && opt->struct_size != sizeof(pndf_project_options4) &&
            opt->struct_size != sizeof(pndf_project_options5) && opt->struct_size != sizeof(pndf_project_options6) &&
            opt->struct_size != sizeof(pndf_project_options7) && opt->struct_size != sizeof(pndf_project_options8) &&
            opt->struct_size != sizeof(pndf_project_options9))
            return "pndf_project_options.struct_size is none of sizeof(pndf_project_options), sizeof(pndf_project_options2), "
                   "sizeof(pndf_project_options3), sizeof(pndf_project_options4), sizeof(pndf_project_options5), "
                   "sizeof(pndf_project_options6), sizeof(pndf_project_options7), sizeof(pndf_project_options8), "
                   "sizeof(pndf_project_options9) and sizeof(pndf_project_options10): fill the struct with pndf_default_project_options";
        return why;
    }
    const pndf_project_options10* o10 = (const pndf_project_options10*)opt;
    // what the struct says of itself first: a refusal here has filled nothing
    out = pndf_project_options();
    observed = nullptr;
    tracks = PndfTracks();
    data = PndfData();
    kp = PndfKeypoints();
    cam = PndfCameraTerm();
    len = PndfLengths();
    for (int i = 0; i < PNDF_MAX_SCALES; ++i) len.rate[i] = 1.0f;
    vw.V = 0;
    for (int i = 0; i < PNDF_FK_MAX_VIEWS * 16; ++i) vw.table[i] = 0.f;
    rs = PndfRootSmooth();
    const pndf_project_options8& o8 = o10->base9.base8;
    const int32_t frames = o8.base7.base6.base5.base4.base3.frames;
    if (o10->reserved6 != 0u) return "pndf_project_options10.reserved6 must be 0";
    if (o10->view_flags & ~(uint32_t)PNDF_VIEWS_PER_FRAME) return "pndf_project_options10.view_flags has a bit other than PNDF_VIEWS_PER_FRAME";
    if (o10->n_pose_views < 0 || o10->n_pose_views > PNDF_FK_MAX_VIEWS) return "pndf_project_options10.n_pose_views must lie in 0 .. 8";
    if ((uintptr_t)o10->pose_views & 15) return "pndf_project_options10.pose_views must be 16-byte aligned: a row is fetched in 16-byte quads";
    if (!o10->pose_views && o10->n_pose_views != 0) return "pndf_project_options10.pose_views must not be NULL when n_pose_views is positive";
    if (o10->pose_views && o10->n_pose_views == 0) return "pndf_project_options10.n_pose_views must be positive when pose_views is not NULL";
    if (!o10->pose_views && o10->view_flags != 0u) return "pndf_project_options10.view_flags must be 0 when pose_views is NULL";
    const bool per_frame = (o10->view_flags & PNDF_VIEWS_PER_FRAME) != 0;
    if (per_frame && frames < 2)
        return "pndf_project_options10.view_flags has PNDF_VIEWS_PER_FRAME, so pndf_project_options3.frames must be at least 2 (the table is [frames,V,16])";
    if (o10->pose_views) {
        if (o8.views || o8.n_views != 0)
            return "pndf_project_options10.pose_views is given, so pndf_project_options8.views must be NULL and n_views 0: one table or the other";
        if (!(o8.base7.base6.kp_flags & PNDF_KP_IMAGE)) return "pndf_project_options10.n_pose_views is positive, so pndf_project_options6.kp_flags must have PNDF_KP_IMAGE";
        if (!o8.base7.base6.base5.kp_target) return "pndf_project_options10.n_pose_views is positive, so pndf_project_options5.kp_target must not be NULL";
    }
    pndf_project_options9 base9 = o10->base9;
    base9.base8.base7.base6.base5.base4.base3.base2.base.struct_size = (uint32_t)sizeof(pndf_project_options9);
    if (o10->pose_views) {      // the intrinsics of base6 are not read: whatever they hold is not refused
        base9.base8.base7.base6.fx = base9.base8.base7.base6.fy = 1.f;
        base9.base8.base7.base6.cx = base9.base8.base7.base6.cy = 0.f;
    }
    if (const char* why = pndf_check_project_options9(&base9.base8.base7.base6.base5.base4.base3.base2.base, B, nj, out, observed, tracks, data, kp, cam, len, vw, rs)) return why;
    if (o10->pose_views) {
        kp.views = o10->n_pose_views;
        pv.named_table = o10->pose_views;
        pv.V = o10->n_pose_views;
        pv.frames = per_frame ? frames : 0;
        if (kp.any()) pv.table = o10->pose_views;
    }
    return nullptr;
}

// What the entry point adds to that checker, knowing B and the poses: every step reads pose_views, so it may share memory with nothing
// the steps write -- q_out, root when a root weight is positive, bone_scale when nu_len > 0.  nullptr, or the reason.  The arrays are
// compared as the struct names them.
inline const char* pndf_check_pose_views_apart(const PndfPoseViews& pv, const PndfCameraTerm& cam, const PndfLengths& len, const float* q_out,
                                               int64_t B, int nj) {
    if (B <= 0 || !pv.named_table) return nullptr;
    const int64_t blocks = pv.frames ? pv.frames : B;
    const uintptr_t r0 = (uintptr_t)pv.named_table, r1 = (uintptr_t)(pv.named_table + blocks * pv.V * 16);
    auto meets = [&](const float* p, int64_t floats) { return p && (uintptr_t)p < r1 && r0 < (uintptr_t)(p + floats); };
    if (meets(q_out, B * nj * 4)) return "pndf_project_options10.pose_views must not overlap q_out";
    if ((cam.nu_rot > 0.f || cam.nu_trans > 0.f) && meets(cam.named_root, B * 7))
        return "pndf_project_options10.pose_views must not overlap pndf_project_options6.root: every step writes the root";
    if (len.nu_len > 0.f && meets(len.named_scale, len.named_floats))
        return "pndf_project_options10.pose_views must not overlap pndf_project_options7.bone_scale: every step writes the scales";
    return nullptr;
}

// The host tables of validated keypoints as the step functions of pndf_fk.h take them: kp_joint and kp_offset with their defaults
// filled in (keypoint k is joint k; zeros).  T: anything with rest [96], kpj [64] and kpo [192] -- the kernel's argument struct, the
// host twin's local copy.
template <class T>
inline void pndf_fill_keypoint_tables(T& t, const PndfKeypoints& kp, int nj) {
    for (int i = 0; i < 3 * nj; ++i) t.rest[i] = kp.rest[i];
    for (int k = 0; k < kp.K; ++k) {
        t.kpj[k] = kp.joint ? kp.joint[k] : k;
        for (int a = 0; a < 3; ++a) t.kpo[3 * k + a] = kp.offset ? kp.offset[3 * k + a] : 0.f;
    }
}

// the defaults give the plain step of pndf_project, whatever else the struct says
inline bool pndf_project_options_plain(const pndf_project_options& o) {
    return o.step_size == 1.0f && o.renorm == PNDF_RENORM_NONE && !(o.tol > 0.0f);
}

// mode / renorm / step_size / tol of a kernel-argument struct (PndfKernelArgs, PndfGenericArgs) for a launch in `mode` with the
// validated options `popt` (null = none): the options' own mode only when one of them differs from its default, else the plain
// loop, bit for bit
template <class Args>
inline void pndf_fill_step_options(Args& a, int mode, const pndf_project_options* popt) {
    const bool plain = !popt || mode != MODE_PROJECT || pndf_project_options_plain(*popt);
    a.mode = plain ? mode : MODE_PROJECT_OPT;
    a.renorm = plain ? 0 : popt->renorm;
    a.step_size = plain ? 1.0f : popt->step_size;
    a.tol = plain ? 0.0f : popt->tol;
}
