"""CPU: the inputs of tests/test_landing_gpu.py say what they are meant to say.  The seed-21 repeat genome (1 Mbp, five
records named `chrN test`) under random_annotation(default_rng(31), 5, 3000, span=250_000): how many places the brute force
finds, how many of them lie in an exon, how often each status occurs, and that the 32 guides landing_util picks carry
every one of them -- a guide's own places are landings of the guide (its off-target at distance 0)."""
import numpy as np

import landing_util as mu
import locate_util as lu
import transcripts_util as tu


def test_the_repeat_case_covers_every_status():
    fasta, records, truth, gff, hits, guides = mu.repeat_case()
    assert [n for n, _ in records] == [b"chr%d test" % r for r in range(5)]
    assert sum(len(s) for _, s in records) == 1_000_000
    assert [mu.query_name(n) for n, _ in records] == [b"chr%d" % r for r in range(5)]
    assert len(truth) == 187_837
    assert int((hits["hit"] > 0).sum()) == 24_881
    assert [int((hits["status"] == s).sum()) for s in (0, 2, 3)] == [182_576, 2_623, 2_638]
    assert not np.any(hits["status"] == 1)
    assert int(np.unique(truth["site"], return_counts=True)[1].max()) <= 42  # long runs come from the runs genome
    # the picked guides: 8 per group, distinct, and their own places show every answer
    assert len(guides) == 32 and len(set(guides.tolist())) == 32
    own = hits[np.isin(truth["site"], guides)]
    assert set(own["status"].tolist()) == {0, 2, 3}
    assert np.any(own["hit"] > 0) and np.any(own["hit"] == 0)
    by_site = {int(s): hits[truth["site"] == s] for s in guides}
    groups = [guides[0:8], guides[8:16], guides[16:24], guides[24:32]]
    assert all(np.any((by_site[int(s)]["status"] == 0) & (by_site[int(s)]["hit"] > 0)) for s in groups[0])
    assert all(np.any((by_site[int(s)]["status"] == 0) & (by_site[int(s)]["hit"] == 0)) for s in groups[1])
    assert all(np.any(by_site[int(s)]["status"] == 2) for s in groups[2])
    assert all(np.any(by_site[int(s)]["status"] == 3) for s in groups[3])


def test_the_join_on_hand_made_records():
    """join() and profile() on records written by hand: order, ranks, repeated sites, an absent site, the two hit forms."""
    fasta, words = mu.runs_genome(counts=[2, 3, 1], names=(b" r0 x", b"r.1", b"r2"))
    records = lu.parse([fasta])
    truth = lu.brute_force(records)
    gff = tu.gff_line("r0", "mRNA", 1, 10, "ID=t;Parent=g") + tu.gff_line("r0", "exon", 1, 45, "ID=e;Parent=t") + \
        tu.gff_line("r_1", "mRNA", 1, 10, "ID=u;Parent=g") + tu.gff_line("r_1", "exon", 1, 1000, "ID=f;Parent=u")
    hits = mu.location_hits(records, truth, tu.Model(gff))
    import crackling_amd as ca
    sites = ca.encode_guides([w[:20] for w in words] + ["A" * 20])
    recs = np.zeros(5, dtype=ca.OFFTARGET_DTYPE)
    recs["site"] = [sites[0], sites[3], sites[1], sites[0], sites[2]]
    recs["guide"] = [0, 0, 0, 2, 2]
    recs["dist"] = [0, 1, 2, 1, 0]
    recs["occ"] = [2, 9, 3, 2, 1]
    offs = np.array([0, 3, 3, 5])
    offsets, rows, cnt = mu.join(3, offs, recs, truth, hits)
    assert cnt.tolist() == [2, 0, 3, 2, 1] and offsets.tolist() == [0, 5, 5, 8]
    assert rows["rank"].tolist() == [0, 0, 2, 2, 2, 0, 0, 1] and rows["guide"].tolist() == [0] * 5 + [2] * 3
    starts = mu.run_starts([2, 3, 1])
    assert rows["pos"].tolist() == [starts[0], starts[0] + 23, starts[1], starts[1] + 23, starts[1] + 46, starts[0], starts[0] + 23, starts[2]]
    assert rows["record"].tolist() == [0, 0, 1, 1, 1, 0, 0, 2]
    # r0's exon ends at 45: pos + 1 = 18 is inside, 41 is inside, ...; the dotted record never matches r_1; r2 is not annotated
    assert rows["hits"]["hit"].tolist() == [1, 1, 0, 0, 0, 1, 1, 0] and starts[0] + 23 + 1 <= 45
    prof = mu.profile(3, recs, cnt, rows)
    assert prof["located"][0].tolist() == [2, 0, 3, 0, 0, 0, 0] and prof["absent"][0].tolist() == [0, 1, 0, 0, 0, 0, 0]
    assert prof["in_exon"][0].tolist() == [2, 0, 0, 0, 0, 0, 0] and prof["located"][1].sum() == 0
    assert prof["located"][2].tolist() == [1, 2, 0, 0, 0, 0, 0] and prof["in_exon"][2].tolist() == [0, 2, 0, 0, 0, 0, 0]
    bare = mu.join(3, offs, recs, truth)[1]
    assert np.all(bare["hits"]["status"] == 1) and np.all(bare["hits"]["first"] == tu.NONE) and np.all(bare["hits"]["hit"] == 0)
    text = mu.records_text(sites[:3], rows, records, True).split(b"\n")
    # (gene g has two mRNA lines, t and u: 1 of 2)
    assert text[0] == b"%s\t%s\t0\t2\t r0 x\t%d\t+\t1/2" % (words[0][:20], words[0][:20], starts[0])
    assert mu.profile_text(sites[:3], prof, 2).split(b"\n")[0] == words[0][:20] + b"\t2\t0\t3\t2\t0\t0\t0\t1\t0"
