"""The rule by which a batched FFTMesh enqueue picks the grid of pass 1, written once in plain Python from the comment of
p1_time_group (csrc/fftmesh_device.h): the time group of an nsteps enqueue is the largest divisor of nsteps in [2, cap], cap = 8
unless the switch MW_P1_TGROUP says otherwise; no such divisor (nsteps = 1, a prime above the cap, cap < 2) = 0, the plain
(GX, nsteps) grid.  tests/test_fftmesh_batch_gpu.py holds mw_debug_pass1_time_group to it, tests/test_emul.py takes the group sizes
of its exhaustive block-map case from it."""

MAX_BATCH = 32      # mw_ocean_max_batch of an FFT-path handle
DEFAULT_CAP = 8     # FmState::p1_tgroup


def time_group(nsteps: int, cap: int = DEFAULT_CAP) -> int:
    divisors = [g for g in range(2, cap + 1) if nsteps % g == 0]
    return max(divisors) if divisors else 0


def plain_grid_sizes(cap: int = DEFAULT_CAP):
    """The batch sizes 1 .. 32 that run pass 1 on the plain 2-D grid."""
    return [ns for ns in range(1, MAX_BATCH + 1) if time_group(ns, cap) == 0]


def group_sizes(nsteps: int, caps=range(2, 9)):
    """Every group size the rule can return for nsteps under the caps the switch is tested with (the plain grid left out)."""
    return sorted({time_group(nsteps, c) for c in caps} - {0})
