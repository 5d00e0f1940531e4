"""bench.py's options, without a GPU: a plain run times one block of --steps steps, --full restores the median of five blocks,
and --dump-outputs belongs to the VGAN_no_kl path."""
import sys

import pytest

import bench


def _parse(monkeypatch, *flags):
    monkeypatch.setattr(sys, "argv", ["bench.py", *flags])
    return bench.parse()


def test_plain_run_times_one_block_full_run_five(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "300", "--warmup", "10")
    assert (a.full, a.repeats, a.steps, a.warmup, a.dump_outputs) == (False, 1, 300, 10, None)
    a = _parse(monkeypatch, "--full")
    assert (a.full, a.repeats) == (True, 5)
    assert _parse(monkeypatch, "--full", "--repeats", "3").repeats == 3
    assert _parse(monkeypatch, "--dump-outputs", "out").dump_outputs == "out"


def test_dump_outputs_needs_the_nokl_path(monkeypatch):
    with pytest.raises(SystemExit):
        _parse(monkeypatch, "--path", "kl", "--dump-outputs", "out")
