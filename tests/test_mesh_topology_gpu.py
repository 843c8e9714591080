"""-m gpu: dgs_amd.mesh_topology.undirected_edges on a HIP device against the CPU result, exactly.  The runs' face order rests on the
device's sort being stable where it is asked to be: a 64 x 64 sheet is large enough to leave the sort's single-block path."""
import pytest
import torch

from test_mesh_topology_cpu import check_edges, sheet

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("n,permute,repeats", [(6, True, False), (64, False, False), (64, True, True)])
def test_undirected_edges_on_the_device(n, permute, repeats):
    from dgs_amd.mesh_topology import half_edges, sorted_edge_keys, undirected_edges
    V, f = sheet(n, permute)
    if repeats:
        f = torch.cat((f, f[::3]))                             # runs of three and four half-edges, far apart in the input
    want = undirected_edges(f)
    got = undirected_edges(f.to(DEV))
    assert all(x.is_cuda and x.dtype == torch.int64 for x in got)
    for x, y in zip(got, want):
        assert torch.equal(x.cpu(), y)
    if n == 6:
        check_edges(f, *(x.cpu() for x in got))
    k2, o2 = sorted_edge_keys(*half_edges(f.to(DEV)))
    assert torch.equal(k2, got[0]) and torch.equal(o2, got[1])
