"""GPU: what the reference's log prints per input file (Crackling.py:254-258), counted during the extraction
(GuideSet.file_counts, issl_guides_file_counts) against a dictionary walk of the same inputs (runlog_model.file_counts);
the arrays the extraction made before are unchanged."""
import numpy as np
import pytest

import crackling_amd as ca
import guides_util as gu
import results_util as ru
import runlog_model as rm
import runlog_util as rl

pytestmark = pytest.mark.gpu


def five_files(seed=4):
    """Five inputs that share guides: records of random bases, some of them copies of a stretch of an earlier input or of
    the input itself, one input without any record of its own guides (all of its guides were seen before) and headers
    that repeat across inputs (a record whose name was recorded does not count)."""
    rng = np.random.default_rng(seed)
    rand = lambda n: "".join(rng.choice(list("ACGT"), n))  # noqa: E731
    pool, files = [], []
    for f in range(5):
        records = []
        for r in range(4):
            kind = rng.integers(0, 4)
            if f == 3 or (kind == 0 and pool):
                seq = pool[rng.integers(0, len(pool))]
                seq = seq[int(rng.integers(0, 40)):]
            elif kind == 1:
                seq = rand(150)
                seq = seq + seq[20:90]                                   # guides repeated inside one record
            else:
                seq = rand(int(rng.integers(120, 400)))
            pool.append(seq)
            name = f"shared {r}" if rng.integers(0, 5) == 0 else f"file {f} record {r}"
            records.append(f">{name}\n{seq}\n")
        files.append("".join(records).encode())
    return files


def running(counts):
    """[identified, duplicates, second_seen, first_seen] per input -> the log's [identified, duplicates, repeated, distinct]."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    return np.column_stack([counts[:, 0], counts[:, 1], np.cumsum(counts[:, 2]), np.cumsum(counts[:, 3])]).tolist()


MULTI = [p.read_bytes() for p in sorted((rl.GOLDEN / "multi").iterdir(), reverse=True)]  # the multi-file golden, as it is read


@pytest.mark.parametrize("blobs", [MULTI, five_files(), five_files(8)[:2], [ru.crafted_fasta(60, 3)],
                                   [b">none\nATATATATATATATATATATATATATATAT\n", ru.crafted_fasta(60, 3), b">empty\n"]],
                         ids=["multi-file golden", "five files", "two files", "one file", "inputs without a match"])
def test_file_counts_against_a_dictionary_walk(blobs):
    want = rm.file_counts(blobs)
    with ca.GuideSet.extract(blobs) as gs:
        got = gs.file_counts
        assert got.shape == (len(blobs), 4) and running(got) == want
        assert got[:, 0].sum() == gs.n_matches and got[:, 3].sum() == gs.n_guides
        assert got[:, 2].sum() == gs.n_guides - gs.n_unique
        gu.check_set(gs, gu.parse(blobs), gu.brute_force(gu.parse(blobs)))  # the arrays of before, field by field
    if len(blobs) == 5:
        assert all(w[1] > 0 for w in want[1:]) and want[-1][2] > want[0][2] > 0, "duplicates inside and across the inputs"


def test_more_inputs_than_the_kernel_keeps_in_lds():
    """300 inputs of one record each, every third a copy of the one before: the counters of the inputs from 256 on are
    added in global memory."""
    rng = np.random.default_rng(12)
    blobs = []
    for f in range(300):
        seq = blobs[-1].split(b"\n")[1].decode() if f % 3 == 2 else "".join(rng.choice(list("ACGT"), 90))
        blobs.append(f">r{f}\n{seq}\n".encode())
    with ca.GuideSet.extract(blobs) as gs:
        assert running(gs.file_counts) == rm.file_counts(blobs)
        assert gs.file_counts[256:, 0].sum() > 0


def test_an_input_beyond_the_last_is_refused():
    import ctypes as C
    with ca.GuideSet.extract([ru.crafted_fasta(20, 1)]) as gs:
        out = (C.c_uint32 * 4)()
        assert ca.lib.issl_guides_file_counts(gs._h, 0, out) == 0 and out[0] == gs.n_matches
        assert ca.lib.issl_guides_file_counts(gs._h, 1, out) == -1
        assert ca.lib.issl_guides_file_counts(gs._h, 0, None) == -1
