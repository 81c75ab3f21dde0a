"""Inputs of the chain-selection tests (tests/test_qa_eval_host.py on the CPU, tests/test_reader_select_gpu.py on the device): fp16 rank
and span scores of many questions under one offsets array. numpy only; importing this file needs no device."""
import numpy as np

SWEEP = [0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 1]                     # predict()'s combination factors
SIXTEEN = [0, 0.05, 0.1, 0.2, 0.25, 0.3, 0.4, 0.5, 0.55, 0.6, 0.7, 0.75, 0.8, 0.9, 0.95, 1]
BASE_SIZES = (1, 2, 3, 5, 8, 50)
EDGE_SIZES = (0, 63, 64, 65, 100, 129, 1000)                                   # empty, around one wave, several strides of a lane


def sizes_for(rng, n_q, edge_repeats=2):
    """n_q segment sizes drawn from BASE_SIZES with every EDGE_SIZES entry planted edge_repeats times at random places: mixed and adjacent."""
    sizes = rng.choice(BASE_SIZES, n_q)
    at = rng.choice(n_q, len(EDGE_SIZES) * edge_repeats, replace=False)
    sizes[at] = np.tile(EDGE_SIZES, edge_repeats)
    return sizes


def offsets_of(sizes):
    q = np.zeros(len(sizes) + 1, np.int64)
    q[1:] = np.cumsum(sizes)
    return q


def tie_heavy(seed, n_q, edge_repeats=2):
    """Scores on the grid -2 .. 2 in steps of 0.5: keys tie under most factors, so the order the earlier sorts left decides."""
    rng = np.random.default_rng(seed)
    q = offsets_of(sizes_for(rng, n_q, edge_repeats))
    grid = np.arange(-2, 2.5, 0.5).astype(np.float16)
    return rng.choice(grid, q[-1]), rng.choice(grid, q[-1]), q


def low_tie(seed, n_q, edge_repeats=2):
    """fp16 of N(0, 2^2): few ties, keys that round."""
    rng = np.random.default_rng(seed)
    q = offsets_of(sizes_for(rng, n_q, edge_repeats))
    return (rng.standard_normal(q[-1]) * 2).astype(np.float16), (rng.standard_normal(q[-1]) * 2).astype(np.float16), q
