"""``python -m sac_eo.train --alg_type mbrl --mf_algo ppo --runs 2 --pack_runs`` on the device against the same
command without ``--pack_runs`` (the runs one after another, each on its own engine), at the loop sizes of
tests/test_mbrl_config.py: every learner of the packed engine computes what its own engine computes, so each
run's log -- train values, final weights, parameters -- equals its serial run's in every key but ``time_*``."""
import numpy as np
import pytest

from test_mbrl_config import ENSEMBLE_KEYS, TRAIN_KEYS, _argv
from test_packed_mbrl_host import _same

pytestmark = pytest.mark.gpu


def test_packed_runs_equal_the_serial_runs_on_the_device(gpu_available, tmp_path):
    from sac_eo.common.logger import load_log
    from sac_eo.train import main
    serial = load_log(main(_argv(tmp_path, ("--runs", "2"))))
    packed = load_log(main(_argv(tmp_path, ("--runs", "2", "--pack_runs"))))
    assert len(serial) == len(packed) == 2
    for r in range(2):
        assert set(packed[r]["train"]) == set(TRAIN_KEYS + ENSEMBLE_KEYS) and set(serial[r]) == set(packed[r])
        for part in ("train", "final", "param"):
            _same(serial[r][part], packed[r][part], f"run{r}.{part}")
        assert all(np.all(np.isfinite(w)) for w in packed[r]["final"]["actor_weights"])
        assert np.any(np.asarray(packed[r]["train"]["kl_agg"]) > 0)                 # the policy moved
    # two different runs, not one run twice
    assert not np.array_equal(np.asarray(packed[0]["train"]["ent"]), np.asarray(packed[1]["train"]["ent"]))
