// nx_wavefront_detail.hip — the DETAIL instances of the material kernels (normal and roughness maps: nxhip_set_material_detail).
//
// The kernels are the templates of nx_wavefront.h, compiled here for DETAIL = true and for nothing else: a translation unit of its
// own, so that the instances of contexts without detail maps (nx_wavefront.hip) are built with the neighbours they had and the build
// compiles the two families side by side (profiles/analytic_lights.txt section 3 records what doubling the instances of ONE unit did
// to the build; profiles/detail_maps.txt what this one costs).  DETAIL implies the general material launch: there is no NO_MAPS form.
// This unit holds instances and their lookups only (the shading-frame test hook: nx_hook_kernels.hip).
#define NX_KERNEL_TU 1
#include "nx_wavefront.h"

namespace nxd {

// (the instances only the pass graphs of a context with detail maps launch — nxhip_render.hip pass_flavor, kFlavorDetail)
using DetailSets = Instances<kMfPower | kMfAnalytic | kMfDetail, kMfAnalytic | kMfDetail, kMfPower | kMfDetail, kMfDetail>;
namespace wavefront_detail {
const void* shade(int type, unsigned set) { return shade_instance<DetailSets, NX_MAT_DIFFUSE, NX_MAT_DIELECTRIC, NX_MAT_PLASTIC, NX_MAT_CONDUCTOR>(type, set); }
// (the SCAN material launch alone has TREE forms: nx_variants.h)
using DetailScanSets = Instances<kMfTree | kMfPower | kMfAnalytic | kMfDetail, kMfPower | kMfAnalytic | kMfDetail, kMfAnalytic | kMfDetail, kMfTree | kMfPower | kMfDetail, kMfPower | kMfDetail, kMfDetail>;
const void* shade_scan(unsigned set) { return shade_scan_instance<DetailScanSets>(set); }
const void* tail(unsigned set) { return tail_instance<DetailSets>(set); }
}  // namespace wavefront_detail

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_wavefront_detail() { return layout_stamp(); }

}  // namespace nxd
