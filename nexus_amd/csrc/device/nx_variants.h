// nx_variants.h — the names of the compile-time kernel instances: which features of a scene a kernel was compiled for.
//
// A feature is a template instance, not a run-time branch: a context without the feature launches the kernels it always did.  A kernel
// template takes ONE set of these bits; the templates of the material kernels stand in a header (nx_wavefront.h), the kernel units that
// include it (nx_wavefront.hip, nx_wavefront_detail / _metal / _solid.hip) list the sets they compile and look an instance up by its set
// (a set nobody compiled yields no kernel), the host derives the set of a launch from the pass flavor (nxhip_render.hip material_features,
// trace_features).  Plain constexpr: kernel units and host units both include this.  What each feature means, and what it measured,
// stands at the code that reads it (nx_trace.hip trace_kernel; nx_wavefront.h next_event_estimation, shade_path, shade_scan_kernel).
// Not to be confused with the run-time launch flags of nx_device.h (kTraceScanFlag, kTraceEntryFlag, kTraceThinFlag: bits of a launch's
// bounce argument).
#pragma once

namespace nxd {

// ---- material features: next_event_estimation, shade_path, the material kernels, the tail kernel, the medium's scatter kernel ----------
constexpr unsigned kMfPower = 1u;      // POWER: the mesh-light sample comes from the light table (NXHIP_LIGHTS_POWER)
constexpr unsigned kMfNoMaps = 2u;     // NO_MAPS: no material names a diffuse or an emissive map, and there is no environment map
constexpr unsigned kMfAnalytic = 4u;   // ANALYTIC: the context has analytic lights
constexpr unsigned kMfDetail = 8u;     // DETAIL: some material names a normal or a roughness map
constexpr unsigned kMfMetal = 16u;     // METAL: some material is an NX_MAT_METALROUGH
constexpr unsigned kMfSolid = 32u;     // SOLID: some material is NX_ALPHA_MASK or NX_ALPHA_OPAQUE
constexpr unsigned kMfTree = 64u;      // TREE: ... and by the shading point's position, from the light tree (NXHIP_LIGHT_IMPORTANCE_POSITION)
constexpr unsigned kMfAll = 127u;

// SOLID => METAL => DETAIL => not NO_MAPS: the later families were built on the earlier ones' records (a SOLID instance knows all five
// material types and reads a detail record; METAL's metalness comes with the roughness map's lookup; DETAIL has no map-free form).
// TREE => POWER and not NO_MAPS: the tree refines the table's mode (its leaves are the table's entries), and it has no map-free form.
constexpr bool material_set_ok(unsigned f)
{
    return (f & ~kMfAll) == 0u && (!(f & kMfSolid) || (f & kMfMetal)) && (!(f & kMfMetal) || (f & kMfDetail)) && (!(f & kMfDetail) || !(f & kMfNoMaps)) &&
           (!(f & kMfTree) || ((f & kMfPower) && !(f & kMfNoMaps)));
}
// ... and the smallest such set over `f`: what a scene with the features `f` launches
constexpr unsigned material_closure(unsigned f)
{
    if (f & kMfSolid) f |= kMfMetal;
    if (f & kMfMetal) f |= kMfDetail;
    if (f & kMfDetail) f &= ~kMfNoMaps;
    if (f & kMfTree) f = (f | kMfPower) & ~kMfNoMaps;
    return f;
}

// What a kernel family leaves out of the rule, because something else says it or because it never gets there:
//   shade_kernel (classic pipeline): its TYPE says what METAL would — an instance of NX_MAT_METALROUGH is a DETAIL instance, the four
//     reference types know nothing of the fifth — and the pipeline has no map-free form and no TREE one (the setting is ignored there);
//   tail_kernel: no map-free form, no SOLID one and no TREE one (no tail kernel under alpha modes or the light tree: nxhip_render.hip tail_bounce);
//   medium_scatter_kernel: shades no surface — it knows the light sample's three features and the fifth type's hit code;
//   logic_kernel: the analytic lights' count in the weighted miss, nothing else.
constexpr unsigned kMfShadeReads = kMfPower | kMfAnalytic | kMfDetail | kMfSolid;
constexpr unsigned kMfTailReads = kMfPower | kMfAnalytic | kMfDetail | kMfMetal;
constexpr unsigned kMfMediumReads = kMfPower | kMfAnalytic | kMfMetal | kMfTree;
constexpr unsigned kMfLogicReads = kMfAnalytic;
constexpr bool shade_set_ok(unsigned f, bool metalType) { return (f & ~kMfShadeReads) == 0u && material_set_ok(f | ((metalType || (f & kMfSolid)) ? kMfMetal : 0u)); }
constexpr bool tail_set_ok(unsigned f) { return (f & ~kMfTailReads) == 0u && material_set_ok(f); }
constexpr bool medium_set_ok(unsigned f) { return (f & ~kMfMediumReads) == 0u && (!(f & kMfTree) || (f & kMfPower)); }

// ---- trace features: trace_kernel ------------------------------------------------------------------------------------------------
constexpr unsigned kTfAnyHit = 1u;     // ANY_HIT: shadow rays (else closest hit)
constexpr unsigned kTfCounting = 2u;   // STATS: the counting variant (nxhip_set_trace_stats)
constexpr unsigned kTfEntry = 4u;      // ENTRY: the primary launch of a pass with entry points
constexpr unsigned kTfIdentity = 8u;   // IDENTITY: every instance of the scene carries the identity
constexpr unsigned kTfTransmit = 16u;  // TRANSMIT: shadow rays carry a transmittance
constexpr unsigned kTfAlphaTest = 32u; // ALPHA_TEST: some material is NX_ALPHA_MASK
constexpr unsigned kTfAll = 63u;

// IDENTITY has no counting form (the counting variants keep the flag of DeviceState::sceneFlags — and the entry install, so ENTRY has
// none either); ENTRY is the closest-hit primary launch's; TRANSMIT: the general any-hit instance and its counting variant only;
// ALPHA_TEST: the general instances and their counting variants only.
constexpr bool trace_counting_ok(unsigned f) { return !(f & kTfCounting) || !(f & (kTfIdentity | kTfEntry)); }
constexpr bool trace_entry_ok(unsigned f) { return !(f & kTfEntry) || !(f & kTfAnyHit); }
constexpr bool trace_transmit_ok(unsigned f) { return !(f & kTfTransmit) || ((f & kTfAnyHit) && !(f & (kTfEntry | kTfIdentity))); }
constexpr bool trace_alpha_test_ok(unsigned f) { return !(f & kTfAlphaTest) || !(f & (kTfEntry | kTfIdentity)); }
constexpr bool trace_set_ok(unsigned f) { return (f & ~kTfAll) == 0u && trace_counting_ok(f) && trace_entry_ok(f) && trace_transmit_ok(f) && trace_alpha_test_ok(f); }

// ---- a family's instances ----------------------------------------------------------------------------------------------------------
// The sets one unit compiles a kernel family for, in the order they are instantiated, and the lookup over them: at(set constant)
// names the instance — the one place that does, so listing a set is compiling it.  A set that is not listed yields nullptr.
template <unsigned F> struct FeatureSet { static constexpr unsigned value = F; };
template <unsigned... SETS> struct Instances {
    template <class At> static const void* find(unsigned set, At at)
    {
        const void* fn = nullptr;
        ((SETS == set ? (void)(fn = at(FeatureSet<SETS>{})) : (void)0), ...);
        return fn;
    }
};

}  // namespace nxd
