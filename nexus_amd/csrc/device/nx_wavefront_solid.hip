// nx_wavefront_solid.hip — the SOLID instances of the material kernels (nxhip_set_material_alpha with a material that is NX_ALPHA_MASK or
// NX_ALPHA_OPAQUE: a hit on such a material never passes through; the rule's one text is shade_path's, nx_wavefront.hip).
//
// The kernels are the templates of nx_wavefront.hip, compiled here for SOLID = true and for nothing else, as nx_wavefront_detail.hip and
// nx_wavefront_metal.hip do for their parameters: every context without such a material launches the kernels it always did.  SOLID
// instances are METAL instances (and with that DETAIL ones: the general material launch, no NO_MAPS form) — those know all five material
// types and read a detail record that may name no map, so one family serves every table; refresh_shade_inst provides the detail records
// while the family is in use.  No tail kernel: tail_bounce is 0 while the family is.
#define NX_WAVEFRONT_INSTANCES_ONLY 1
#include "nx_wavefront.hip"

namespace nxd {

// (the variants only the pass graphs of a context with a MASK or an OPAQUE material launch — nxhip_render.hip frame_levels, materials_solid)
const void* shade_scan_solid_kernel_ptr(bool lightPower, bool analytic)
{
    if (analytic) return lightPower ? (const void*)shade_scan_kernel<true, false, true, true, true, true> : (const void*)shade_scan_kernel<false, false, true, true, true, true>;
    return lightPower ? (const void*)shade_scan_kernel<true, false, false, true, true, true> : (const void*)shade_scan_kernel<false, false, false, true, true, true>;
}

template <int TYPE>
static const void* shade_solid_of(bool lightPower, bool analytic)
{
    if (analytic) return lightPower ? (const void*)shade_kernel<TYPE, true, true, true, true, true> : (const void*)shade_kernel<TYPE, true, false, true, true, true>;
    return lightPower ? (const void*)shade_kernel<TYPE, true, true, false, true, true> : (const void*)shade_kernel<TYPE, true, false, false, true, true>;
}
const void* shade_solid_kernel_ptr(int type, bool lightPower, bool analytic)
{
    switch (type) {
    case NX_MAT_DIFFUSE: return shade_solid_of<NX_MAT_DIFFUSE>(lightPower, analytic);
    case NX_MAT_DIELECTRIC: return shade_solid_of<NX_MAT_DIELECTRIC>(lightPower, analytic);
    case NX_MAT_PLASTIC: return shade_solid_of<NX_MAT_PLASTIC>(lightPower, analytic);
    case NX_MAT_METALROUGH: return shade_solid_of<NX_MAT_METALROUGH>(lightPower, analytic);
    default: return shade_solid_of<NX_MAT_CONDUCTOR>(lightPower, analytic);
    }
}

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_wavefront_solid() { return layout_stamp(); }

}  // namespace nxd
