"""The size bound behind the kernels' 24-bit octant offsets (no device).

A ray's octant copy of the wide tree lies octant x stride float4s into the nodes and
octant x n_top x node_f4 into the LDS top levels; the kernels form both products with a
24-bit multiply, which reads the low 24 bits of each factor.  flatten_scene - the first
step of every context creation, before a device is looked for - therefore refuses a tree
whose stride or top levels reach 2^24 float4s with ZRT_E_UNSUPPORTED, through
zrt::check_octant_offsets; zrt_debug_octant_offsets calls the same function on a shape
given as numbers (a tree of that size has two million nodes per copy).
"""
import pytest

import zraytrace_amd as z

E_UNSUPPORTED = -4
LIM = 1 << 24


@pytest.mark.parametrize("stride, n_top, node_f4", [
    (8, 1, 8),                    # the smallest tree: one node
    (3_700_000, 5, 8),            # the million-triangle mesh's stride
    (LIM - 8, 21, 4),             # the last stride of whole nodes below the bound
    (LIM - 1, (LIM - 1) // 8, 8),  # both just below it
])
def test_shapes_within_the_bound(stride, n_top, node_f4):
    z.debug_octant_offsets(stride, n_top, node_f4)


@pytest.mark.parametrize("stride, n_top, node_f4", [
    (LIM, 5, 8),                  # the stride reaches 2^24
    (LIM + 8, 5, 8),
    (0xfffffff8, 5, 8),           # the largest 32-bit stride
    (1024, LIM // 8, 8),          # the top levels reach 2^24 float4s
    (1024, LIM // 4, 4),
    (1024, 0xffffffff, 8),        # n_top x node_f4 past 32 bits: no wrap-around lets it through
])
def test_shapes_past_the_bound_are_refused(stride, n_top, node_f4):
    with pytest.raises(z.ZrtError) as e:
        z.debug_octant_offsets(stride, n_top, node_f4)
    assert e.value.code == E_UNSUPPORTED
    assert "2^24" in str(e.value)


def test_shipped_scenes_are_far_below_the_bound(scenes):
    """The launch plans of the mesh scenes exist (flatten_scene accepted their trees)."""
    for which in (2, 3):
        plan = z.debug_launch_plan(scenes(which).view, z.RenderParams(16, 16, 4, 6))
        assert plan["kmode"] == 3
