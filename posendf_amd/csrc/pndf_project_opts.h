// Validation of pndf_project_options (include/posendf_amd.h), shared by pndf_project_ex (pndf_capi.hip) and its host twin
// pndf_project_ex_cpu (pndf_cpu.cpp): the two refuse the same structs with the same text.  And of pndf_project_options2, the options with
// a joint mask, which pndf_skel_project (pndf_skeleton.hip) and pndf_project_ex_cpu take besides, and of pndf_project_options3, the
// options with tracks (pose interpolation inside the step), and of pndf_project_options4, the options with an observation (motion
// denoising inside the step), which the same two take.
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
