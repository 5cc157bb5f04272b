// nx_wavefront_metal.hip — the METAL instances of the material kernels (NX_MAT_METALROUGH, the fifth material type: nxhip_set_materials).
//
// The kernels are the templates of nx_wavefront.h, compiled here for METAL = true and for nothing else, as nx_wavefront_detail.hip does
// for DETAIL (a unit of its own for the same reasons: the other families keep their neighbours, and the build compiles it beside them):
// shade_scan_kernel is one kernel with a switch over the types and its register count is the maximum over its cases, so the
// fifth case exists only in the instances a pass graph picks while some material has the type (kFlavorMetal) — every other context
// launches the kernels it always did.  METAL implies DETAIL (the type's metalness comes from the roughness map's B channel, read in the
// same lookup as the roughness: nx_detail.h) and with it the general material launch: there is no NO_MAPS form.
// Also here: logic_metal_kernel, the classic pipeline's fifth queue (a pass-graph kernel; the type's test hooks: nx_hook_kernels.hip).
#define NX_KERNEL_TU 1
#include "nx_wavefront.h"

namespace nxd {

// The CLASSIC pipeline's fifth material queue (ordered compaction).  logic_kernel stays the reference's: four queues, and a hit of the fifth
// type leaves it as "no kernel" (the path's roulette draw, previous vertex and miss are its business and done there).  This kernel
// runs behind it over the same trace queue and makes the decision of logic_path again for the hits — the same random number, keyed by the
// same slot or pixel — to queue the survivors of type NX_MAT_METALROUGH, in ascending item order like every queue of the mode.
__global__ void __launch_bounds__(kLogicBlock, NX_LOGIC_WAVES) logic_metal_kernel(const DeviceState* __restrict__ S, const int bounce)
{
    Counters* C = S->counters;
    const QueueView in = queue_view(&C->region[0].traceSize[bounce - 1], S->queueShardCap);
    const int size = in.total;
    if ((int)(blockIdx.x * blockDim.x) >= size) return;  // no tile for this workgroup (see logic_kernel)
    const uint32_t frame = S->frame->frameNumber;
    TileAllocator<true, 1, 1> slots;
    slots.init(S, &C->region[0].materialSizeMetal[bounce], 0, 6, bounce, size, &S->counters->region[0].scanTicketMetal[0][bounce]);  // (kind 6: a launch serial nobody else has)
    const MaterialQueue mq = S->materialMetal;
    for (int tile = slots.first_tile(); tile < size; tile = slots.next_tile(tile)) {
        const int index = tile + (int)threadIdx.x;
        bool want[1][1] = {{false}};
        float4 hit = make_float4(0, 0, 0, 0), dirPix = make_float4(0, 0, 0, 0), tpOut = make_float4(0, 0, 0, 0);
        uint32_t inst = 0, pixelIdx = 0;
        if (index < size) {
            const int at = in.slot(index);
            hit = S->trace.hit[at];
            if (hit.x != 1e30f) {
                dirPix = S->trace.rays[0].rayD[at];
                pixelIdx = __float_as_uint(dirPix.w);
                const float4 tp = bounce == 1 ? make_float4(1.0f, 1.0f, 1.0f, 1.0e10f) : S->trace.rays[0].tp[at];
                const uint32_t hitInstance = S->trace.hitInst[at];
                bool miss, survived, needsPrevVertex;
                f3 bg = mk3(0.0f), t = mk3(0.0f);
                const int type = logic_path<false, kMfMetal>(S, bounce, frame, (uint32_t)index, pixelIdx, hit.x, mk3(dirPix.x, dirPix.y, dirPix.z), tp, [&]() { return hitInstance; }, miss, bg,
                                                                survived, t, inst, needsPrevVertex);
                want[0][0] = type == NX_MAT_METALROUGH;
                tpOut = make_float4(t.x, t.y, t.z, tp.w);
            }
        }
        int slot[1][1];
        slots.alloc(want, slot, tile, 0);
        if (want[0][0]) {
            const int sl = slot[0][0];
            mq.hit[sl] = make_float4(__uint_as_float(pixelIdx), hit.y, hit.z, hit.w);
            mq.dirInst[sl] = make_float4(dirPix.x, dirPix.y, dirPix.z, __uint_as_float(inst));
            if (bounce != 1) mq.tp[sl] = tpOut;
        }
    }
}

// (the instances only the pass graphs of a context with an NX_MAT_METALROUGH material launch — nxhip_render.hip pass_flavor, kFlavorMetal)
using MetalSets = Instances<kMfPower | kMfAnalytic | kMfDetail | kMfMetal, kMfAnalytic | kMfDetail | kMfMetal, kMfPower | kMfDetail | kMfMetal, kMfDetail | kMfMetal>;
// (the classic pipeline's material kernel of the fifth type: TYPE says METAL, the set does not — shade_kernel, nx_variants.h)
using MetalShadeSets = Instances<kMfPower | kMfAnalytic | kMfDetail, kMfAnalytic | kMfDetail, kMfPower | kMfDetail, kMfDetail>;
namespace wavefront_metal {
// (the SCAN material launch alone has TREE forms: nx_variants.h)
using MetalScanSets = Instances<kMfTree | kMfPower | kMfAnalytic | kMfDetail | kMfMetal, kMfPower | kMfAnalytic | kMfDetail | kMfMetal, kMfAnalytic | kMfDetail | kMfMetal,
                                kMfTree | kMfPower | kMfDetail | kMfMetal, kMfPower | kMfDetail | kMfMetal, kMfDetail | kMfMetal>;
const void* shade_scan(unsigned set) { return shade_scan_instance<MetalScanSets>(set); }
const void* tail(unsigned set) { return tail_instance<MetalSets>(set); }
const void* shade(int type, unsigned set) { return shade_instance<MetalShadeSets, NX_MAT_METALROUGH>(type, set); }
}  // namespace wavefront_metal
const void* logic_metal_kernel_ptr() { return (const void*)logic_metal_kernel; }

// the device-side layouts this translation unit was compiled with (nx_device.h layout_stamp; compared by nxhip_create)
uint64_t layout_stamp_wavefront_metal() { return layout_stamp(); }

}  // namespace nxd
