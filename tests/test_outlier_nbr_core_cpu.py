"""The shared tail of the detectors on the refined neighbour lists (SubspaceABOD, SubspaceCOF), CPU tier: the fill of the
degenerate rows goes through _NeighborScorer._fill_degenerate, the only place that allocates the fill buffers."""
import inspect

import numpy as np
import pytest
import torch


class _RecordingOps:
    """Stands in for HipOps: records the calls of the two fill entries, every other entry must not be reached."""

    def __init__(self):
        self.calls = []

    def outlier_abod_floor(self, score, value, n_degenerate=None):
        self.calls.append(("floor", score, value, n_degenerate))

    def outlier_cof_ceiling(self, score, value, n_degenerate=None):
        self.calls.append(("ceiling", score, value, n_degenerate))


@pytest.mark.parametrize("name, entry", [("SubspaceABOD", "floor"), ("SubspaceCOF", "ceiling")])
def test_fill_degenerate_is_the_only_place_that_allocates_the_fill_buffers(name, entry, monkeypatch):
    import vgan_amd
    from vgan_amd import outlier
    cls = getattr(vgan_amd, name)
    mask = np.zeros((3, 6), bool)
    mask[0, :2] = mask[1, 2:5] = mask[2, 5] = True
    ens = cls(mask, [0.5, 0.3, 0.2], n_neighbors=2)
    ens.ops, ens._X = _RecordingOps(), torch.zeros(7, 6)
    monkeypatch.setattr(cls, "_neighbors", lambda self, Xq, kdist=None, only=None: iter(()))
    monkeypatch.setattr(cls, "_combine", lambda self, per, fitting: per.double().sum(dim=0))

    _, per = ens._score(None, fitting=True)
    (kind, score, value, ndeg), = ens.ops.calls
    assert kind == entry and score is per and per.shape == (3, 7)
    assert value is ens._fill and value.dtype == torch.float64 and value.shape == (3,)
    assert ndeg is ens._n_degenerate and ndeg.dtype == torch.int32 and ndeg.shape == (3,)

    _, per_new = ens._score(torch.zeros(4, 6), fitting=False)  # applies what the fit stored and allocates nothing
    kind, score, stored, none = ens.ops.calls[1]
    assert kind == entry and score is per_new and per_new.shape == (3, 4) and stored is value and none is None
    assert ens._fill is value and ens._n_degenerate is ndeg

    owners = [c for c in cls.__mro__ if "_fill_degenerate" in vars(c)]
    assert owners == [outlier._NeighborScorer]
    for c in (vgan_amd.SubspaceABOD, vgan_amd.SubspaceCOF):
        src = inspect.getsource(c)
        assert "self._fill =" not in src and "self._n_degenerate =" not in src and "_fill_degenerate(per, fitting" in src
