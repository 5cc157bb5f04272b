"""Worker of tests/test_gpu_blas_refit.py::test_update_blas_device_takes_a_torch_tensor: a process of its own, because torch has to
initialise the GPU before the library does (as in bench.py's distributed path).  The context runs on a torch stream; a torch kernel
on that stream writes the deformed triangle records — a stand-in for a caller's skinning kernel — and nxhip_update_blas_device takes
them from the tensor's data_ptr() with no synchronisation in between.  Writes the refitted nodes and the hits of 20 000 rays."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nexus_amd import capi  # noqa: E402
from tests import deform_meshes as D  # noqa: E402
from tests import scene_helpers as SH  # noqa: E402


def main():
    out_path, m = sys.argv[1], int(sys.argv[2])
    torch.cuda.set_device(0)
    side = torch.cuda.Stream(device=0)
    torch.cuda.set_stream(side)
    placed = np.array(sys.argv[3:19], dtype=np.float32)
    scene = SH.BuiltScene([D.base_grid(m)], [(0, 0, placed)])
    moved = D.deformed_grid(m)
    with capi.Context(64, 64, stream=side.cuda_stream) as ctx:
        scene.upload(ctx)
        before = ctx.trace_batch(D.rays_for(2000, 7))
        # the records as 24 floats each: the base mesh on the device, the displacement added there, on the context's stream
        base = torch.from_numpy(np.frombuffer(scene.meshes[0].tobytes(), dtype=np.float32).copy()).to("cuda")
        delta = torch.from_numpy(np.frombuffer(moved.tobytes(), dtype=np.float32) - np.frombuffer(scene.meshes[0].tobytes(), dtype=np.float32)).to("cuda")
        dev = (base + delta).contiguous()
        assert dev.numel() * 4 == 96 * len(moved)
        ctx.update_blas_device(0, dev.data_ptr(), len(moved))
        nodes, _idx = ctx.read_blas(0, len(moved))
        hits = ctx.trace_batch(D.rays_for(20000, 7))
        held = np.frombuffer(dev.cpu().numpy().tobytes(), dtype=moved.dtype)
        np.savez(out_path, nodes=nodes, hits=hits, held=held, before=before)


if __name__ == "__main__":
    main()
