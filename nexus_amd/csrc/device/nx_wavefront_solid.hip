// nx_wavefront_solid.hip — the SOLID instances of the material kernels (nxhip_set_material_alpha with a material that is NX_ALPHA_MASK or
// NX_ALPHA_OPAQUE: a hit on such a material never passes through; the rule's one text is shade_path's, nx_wavefront.h).
//
// The kernels are the templates of nx_wavefront.h, compiled here for SOLID = true and for nothing else, as nx_wavefront_detail.hip and
// nx_wavefront_metal.hip do for their parameters (and a unit of its own for their reasons: the other families keep their neighbours, the
// build compiles this one beside them): every context without such a material launches the kernels it always did.  SOLID
// instances are METAL instances (and with that DETAIL ones: the general material launch, no NO_MAPS form) — those know all five material
// types and read a detail record that may name no map, so one family serves every table; refresh_shade_inst provides the detail records
// while the family is in use.  No tail kernel: tail_bounce is 0 while the family is.
#define NX_KERNEL_TU 1
#include "nx_wavefront.h"

namespace nxd {

// (the instances only the pass graphs of a context with a MASK or an OPAQUE material launch — nxhip_render.hip pass_flavor, kFlavorSolid)
using SolidSets = Instances<kMfTree | kMfPower | kMfAnalytic | kMfDetail | kMfMetal | kMfSolid, kMfPower | kMfAnalytic | kMfDetail | kMfMetal | kMfSolid,
                            kMfAnalytic | kMfDetail | kMfMetal | kMfSolid, kMfTree | kMfPower | kMfDetail | kMfMetal | kMfSolid, kMfPower | kMfDetail | kMfMetal | kMfSolid,
                            kMfDetail | kMfMetal | kMfSolid>;
// (the classic pipeline's material kernels, all five types: TYPE says METAL, the set does not — shade_kernel, nx_variants.h)
using SolidShadeSets = Instances<kMfPower | kMfAnalytic | kMfDetail | kMfSolid, kMfAnalytic | kMfDetail | kMfSolid, kMfPower | kMfDetail | kMfSolid, kMfDetail | kMfSolid>;
namespace wavefront_solid {
const void* shade_scan(unsigned set) { return shade_scan_instance<SolidSets>(set); }
const void* shade(int type, unsigned set)
{
    return shade_instance<SolidShadeSets, NX_MAT_DIFFUSE, NX_MAT_DIELECTRIC, NX_MAT_PLASTIC, NX_MAT_METALROUGH, NX_MAT_CONDUCTOR>(type, set);
}
}  // namespace wavefront_solid

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_wavefront_solid() { return layout_stamp(); }

}  // namespace nxd
