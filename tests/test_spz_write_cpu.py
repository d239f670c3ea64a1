"""CPU-only check of st_write(): without a device it fails loudly (no host encoder stands in) and writes nothing."""
import os

import numpy as np
import pytest


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="a GPU is present")
def test_st_write_without_a_device_is_loud(tmp_path):
    import rcppml_amd
    from rcppml_amd import _abi
    from rcppml_amd.data import simulate_nmf_sparse
    A, _, _ = simulate_nmf_sparse(30, 40, 3, 0.3, seed=1)
    with pytest.raises(_abi.BackendError, match="no HIP device"):
        rcppml_amd.st_write(A, tmp_path / "a.spz")
    assert not (tmp_path / "a.spz").exists()
