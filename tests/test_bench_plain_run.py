"""bench.py on the CPU: a plain run selects no side leg (they run with --full), and the waveforms that ClipMaker makes in
spawned processes are bit-identical to the serial synth_utterances / synth_workload ones."""
import numpy as np
import pytest

import bench


def test_plain_run_runs_no_side_leg():
    args = bench.parse(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not args.full
    for world, rank in ((1, 0), (2, 0), (2, 1)):
        assert not any(bench.side_legs(args, world, rank).values()), (world, rank)


def test_full_run_keeps_every_side_leg():
    args = bench.parse(["--full"])
    assert bench.side_legs(args, 1, 0) == {"phases": True, "through_plugin": True, "cpu": True, "other_workloads": True}
    # N > 1: every rank runs the plugin leg, rank 0 the phase step; the CPU and other-workload legs are N = 1 only
    assert bench.side_legs(args, 2, 0) == {"phases": True, "through_plugin": True, "cpu": False, "other_workloads": False}
    assert bench.side_legs(args, 2, 1) == {"phases": False, "through_plugin": True, "cpu": False, "other_workloads": False}
    off = bench.parse(["--full", "--no-phases", "--no-through-plugin", "--no-cpu-baseline", "--no-other-workloads"])
    assert not any(bench.side_legs(off, 1, 0).values())
    assert not any(bench.side_legs(bench.parse(["--full", "--workload", "c4"]), 1, 0).values())
    tiny = bench.side_legs(bench.parse(["--full", "--tiny"]), 1, 0)
    assert tiny == {"phases": False, "through_plugin": False, "cpu": True, "other_workloads": False}


def test_explicit_leg_flags():
    assert bench.parse(["--cpu-baseline-full"]).full
    legs = bench.side_legs(bench.parse(["--through-plugin", "--tiny"]), 1, 0)
    assert legs == {"phases": False, "through_plugin": True, "cpu": False, "other_workloads": False}


@pytest.mark.parametrize("workers", [1, 2])
@pytest.mark.parametrize("workload", ["c2", "c2s"])
def test_clip_maker_matches_serial_synthesis(workload, workers):
    _, text_lens, n_audio = bench.WORKLOADS[workload]
    count, steps = 3, 4          # more steps than ring slots: every slot is refilled
    maker = bench.ClipMaker([bench.clip_seeds(workload, s * count, count) for s in range(steps)], workers=workers, depth=2)
    try:
        for s in range(steps):
            got = maker.take(s)
            if workload == "c2":
                want, _ = bench.synth_utterances(s * count, count, 32000)
            else:
                want, _ = bench.synth_workload(s * count, count, 32000, text_lens, n_audio, bench.N_AUDIO_TOK)
            assert got.dtype == np.float32 and got.shape == (count * n_audio, bench.CLIP_SAMPLES)
            assert np.array_equal(got, want), (workload, s)
    finally:
        maker.close()


def test_inputs_without_audio_are_the_same_ids():
    _, ids = bench.synth_utterances(5, 2, 32000)
    wav, ids2 = bench.synth_utterances(5, 2, 32000, audio=False)
    assert wav is None and np.array_equal(ids, ids2)
    _, text_lens, n_audio = bench.WORKLOADS["c5"]
    _, pr = bench.synth_workload(5, 3, 32000, text_lens, n_audio, bench.N_AUDIO_TOK)
    wav, pr2 = bench.synth_workload(5, 3, 32000, text_lens, n_audio, bench.N_AUDIO_TOK, audio=False)
    assert wav is None and pr == pr2
