"""Scene assembly shared by tests/test_trace_reference_cpu.py, tests/test_gpu_trace_reference.py and tests/test_gpu_trace_edits.py (tests/trace_reference.py
itself imports nothing of the product)."""
import numpy as np


def build_scene(instances):
    """instances: [(triangles (n, 3, 3) float32, 16-float transform or None = identity)], one mesh and one object each."""
    from gpuspectral_amd import scenes

    b = scenes.SceneBuilder()
    mat = b.diffuse((0.5, 0.5, 0.5))
    for tris, transform in instances:
        pos = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
        nrm = np.zeros_like(pos)
        nrm[:, 1] = 1.0
        b.add_object(b.add_mesh(pos, nrm), scenes.trs() if transform is None else transform, mat)
    return b.build()
