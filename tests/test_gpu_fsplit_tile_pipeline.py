"""dx_kernel (csrc/fsplit.hip) pipelines its tile loop across tiles: row half 1 of tile t is finished in the iteration of tile
t + 1, the input images and row factors rotate through three LDS slots and the sm images through two, and the last tile's row
half 1 runs after the loop. Every slot phase and tile count per workgroup from 1 to 5 is taken here against the float64 oracle
(tests/test_gpu_fsplit.py covers 1-2 tiles and the full 4096 x 5 size).
These compare the mean over a set; tile by tile through 33 ordinals: tests/test_gpu_fsplit_tiles.py, docs/fsplit_tile_parity.md."""
import numpy as np
import pytest
import torch

from tests.gpu_util import need_gpu, t
from tests.test_gpu_fset import _batch
from tests.test_gpu_fsplit import _errors_vs_oracle, _untie
from tests.test_gpu_mlp import _perturbed_group

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("S,tiles,M", [(4, 4, 1), (3, 3, 2), (4, 5, 1)])
def test_split_set_learner_with_several_tiles_per_workgroup_matches_oracle(S, tiles, M):
    need_gpu()
    J = max(1, torch.cuda.get_device_properties(0).multi_processor_count // M)  # workgroups per set (fsplit.hip: make_plan)
    P = (tiles - 1) * J + max(1, J // 3)  # the first J // 3 workgroups of a set take `tiles` tiles, the others one fewer
    conf, grp = _perturbed_group(M, S=S, seed=71)
    rs = np.random.RandomState(72)
    n = P * M
    s, a, r, s2 = _batch(rs, n, S)
    _untie(grp, M, S, s, a)
    losses = torch.zeros(M, 2, device="cuda")
    g = grp.learn_set_split(t(s), t(a), t(r), t(s2), n, losses=losses)
    torch.cuda.synchronize()
    assert torch.isfinite(g).all()
    errs, _ = _errors_vs_oracle(grp, g, s, a, r, s2, P, M, range(M), losses=losses)
    assert not errs, errs
