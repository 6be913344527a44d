"""bench.py --dump-outputs: the arrays written for a Result (host only, no GPU work)."""
import os
import types

import numpy as np

import bench


def _result():
    return types.SimpleNamespace(verdict="DEPTH_LIMIT", generated=1348469533, distinct=54426066, depth=3, left_on_queue=7,
                                 generated_in_model=589936128, levels=[(1, 6, 0.1), (6, 30, 0.2), (23, 90, 0.3)],
                                 actions={"Timeout": [9, 4], "AppendEntries": [5, 0], "Restart": [3, 3]})


def test_dump_outputs_arrays(tmp_path, raftmc):
    d = str(tmp_path / "out")
    meta = bench.dump_outputs(d, _result(), raftmc.raftmc.VERDICTS, False)
    assert sorted(os.listdir(d)) == ["action_generated.npy", "level_states.npy", "summary.npy"]
    assert meta["actions"] == ["AppendEntries", "Restart", "Timeout"]
    arrays = {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["summary"].tolist() == [5, 1348469533, 54426066, 3, 7, 589936128]
    assert arrays["level_states"].tolist() == [1, 6, 23]
    assert arrays["action_generated"].tolist() == [5, 3, 9]
    assert meta["arrays"] == {k: len(v) for k, v in arrays.items()}


def test_dump_outputs_fifo_order_adds_action_distinct(tmp_path, raftmc):
    """the per-action distinct counts are first-come under -workers N: written for TLC's FIFO order only"""
    d = str(tmp_path / "out")
    bench.dump_outputs(d, _result(), raftmc.raftmc.VERDICTS, True)
    assert np.load(os.path.join(d, "action_distinct.npy")).tolist() == [0, 3, 4]
