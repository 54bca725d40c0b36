"""hspf_routes_backup_srlg_device on seeded random graphs against the model (tests/_backup_srlg_model.py): at most 40 routers and two
LANs, overloaded routers, at most 80 prefixes with up to 4 advertisers, 1 - 6 random group tables; with and without
HSPF_LFA_SRLG_SAFE_REPAIRS and the repairs.  tests/test_host_backup_srlg.py shows on the CPU that these seeds hold every class."""
import pytest

import _backup_srlg_cases as SC
import _backup_srlg_model as BS
from test_gpu_backup_srlg import check

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed", range(SC.RANDOM_SEED, SC.RANDOM_SEED + SC.GPU_GRAPHS))
def test_random_graph_with_groups(spf_ctx, seed):
    g, S, (gp, gr), t = SC.random_case(seed)
    assert len(g[3]) <= 60 and t.n <= 80 and max(int(t.ptr[p + 1]) - int(t.ptr[p]) for p in range(t.n)) <= 4
    check(spf_ctx, SC.Model(g, [S], gp, gr, t), lfa_flags=(0, BS.SAFE_REPAIRS), remotes=(True, False) if seed % 4 == 0 else (True,))
