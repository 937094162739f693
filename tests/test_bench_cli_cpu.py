"""bench.py's command line on the host: a plain run leaves out everything that takes runs of its own after the timed
region; --full brings it back, and the --no-* switches still leave out parts of a --full run."""
import bench

PARTS = ('no_roofline', 'no_selfcheck', 'no_extras', 'no_cpu_baseline')


def test_plain_run_is_lean():
    a = bench.parse_args(['--gpus', '1', '--steps', '20', '--warmup', '5'])
    assert not a.full and (a.steps, a.warmup) == (20, 5)
    assert all(getattr(a, p) for p in PARTS)


def test_full_run_keeps_every_part_unless_switched_off():
    a = bench.parse_args(['--full'])
    assert a.full and not any(getattr(a, p) for p in PARTS)
    b = bench.parse_args(['--full', '--no-cpu-baseline', '--no-extras'])
    assert b.no_cpu_baseline and b.no_extras and not b.no_roofline and not b.no_selfcheck
