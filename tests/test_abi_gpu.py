"""nb_sim_set_tuning's keys of the analysis passes, on a live simulator: every key refuses what lies outside its
allowed values with NB_ERR_INVALID and its own wording, accepts both ends of them, and an unknown key still
reaches the simulator's own refusal."""
import pytest

pytestmark = pytest.mark.gpu

# key -> (the wording of the allowed values, refused values: below, above and off the multiple, lowest, highest)
KEYS = {
    "field_launch_pairs_log2": ("16..40", [15, 41], 16, 40),
    "map_segment_len": ("a multiple of 256 in 256..65536", [0, 65792, 300], 256, 65536),
    "smooth_segment_len": ("a multiple of 256 in 256..65536", [0, 65792, 300], 256, 65536),
    "fof_chunk_len": ("a multiple of 64 in 64..65536", [0, 65600, 100], 64, 65536),
    "fof_cell_boxes": ("0 or 1", [-1, 2], 0, 1),
    "bound_chunk_len": ("a multiple of 64 in 64..1048576", [0, 1048640, 100], 64, 1048576),
    "shape_chunk_len": ("a multiple of 64 in 64..65536", [0, 65600, 100], 64, 65536),
    "bound_tile": ("0, 64 or 256", [-64, 320, 128], 0, 256),
    "knn_span_cells": ("1..8", [0, 9], 1, 8),
    "knn_block_queries": ("1, 2 or 4", [0, 8, 3], 1, 4),
}


def test_tuning_keys_of_the_passes(gpu):
    nb = gpu
    sim = nb.NaiveSim.new(nb.SimParams(particle_num=256), None, lambda sp: nb.inits.uniform_init(sp, seed=3))
    for key, (allowed, refused, lowest, highest) in KEYS.items():
        for value in refused:
            with pytest.raises(nb.NBodyError) as ei:
                sim.set_tuning(key, value)
            assert ei.value.code == 1, (key, value)  # NB_ERR_INVALID
            assert str(ei.value) == f"nbody_hip error 1: {key}: {allowed}, not {value}"
        sim.set_tuning(key, lowest)
        sim.set_tuning(key, highest)
    with pytest.raises(nb.NBodyError) as ei:
        sim.set_tuning("no_such_key", 1)
    assert ei.value.code == 1 and str(ei.value) == "nbody_hip error 1: unknown tuning key 'no_such_key'"
    sim.destroy()
