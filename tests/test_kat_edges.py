"""The edge cases the scene KATs were built for are really in the committed
files.  Every record of tests/golden/kat_{sphere ... texture_image, mesh, world, bounce}.bin is
classified from its inputs and the reference's outputs alone (tests/kat_classes.py:
float32 arithmetic in numpy, no device and no restatement code): each class of the
issue's table holds at least 8 records (a class of the world KAT: the number of records
its generator constructs for it, kat_classes.WORLD_MIN), and each KAT with a hit flag has between a
quarter and three quarters of hits.  This is what lets the bit-exact comparisons
(test_oracle_pins.py, test_device_kat.py) fail where the code can go wrong."""
import numpy as np

import kat_classes as kc
import oracle_bind as ob

MIN_PER_CLASS = 8


def test_kat_edge_classes_populated():
    short, report = [], []
    for name in kc.NEW_KATS:
        rec = ob.read_kat(name)
        assert 512 <= len(rec) <= kc.MAX_RECORDS.get(name, 1024), (name, len(rec))
        counts = {k: int(m.sum()) for k, m in kc.classify(name, rec).items()}
        report.append(f"{name} ({len(rec)} records): " + ", ".join(f"{k}: {v}" for k, v in counts.items()))
        need = kc.MIN_COUNTS.get(name, {})  # (the world KAT: the counts its generator constructs, kat_classes.WORLD_MIN)
        assert set(need) <= set(counts), (name, set(need) - set(counts))
        short += [f"{name}: {k}: {v} < {need.get(k, MIN_PER_CLASS)}" for k, v in counts.items()
                  if v < need.get(k, MIN_PER_CLASS)]
        if name in kc.HIT:
            flag = rec[:, kc.HIT[name]]
            assert np.isin(flag, (0.0, 1.0)).all(), name
            frac = float((flag == 1).mean())
            report.append(f"{name}: hits {frac:.3f}")
            if not 0.25 <= frac <= 0.75:
                short.append(f"{name}: hit fraction {frac:.3f}")
        if name == "mesh":  # the NaN-bound scan is wave-cooperative: every wave mixes NaN and finite lanes
            bad = kc.mesh_nan_waves(rec)
            if bad:
                short.append(f"mesh: records {bad} onwards: a wave of 64 with NaN bounds only")
        if name == "bounce":  # a wave of k_paths mixes the families: so does every group of 64 consecutive records
            assert 1536 <= len(rec), len(rec)
            if counts[kc.BOUNCE_WALK_MISSES]:  # the last-branch classes rest on the classifier's own walk of every loop
                short.append(f"bounce: the LCG walk misses {counts[kc.BOUNCE_WALK_MISSES]} records with a mixture loop")
            first = kc.bounce_waves_mixed(rec)
            if first >= 0:
                short.append(f"bounce: records {first} to {first + 63} lack a family")
        if name == "world":  # the share of records the device test compares on hit and t alone is capped
            share = float(kc.world_t_only(rec).mean())
            report.append(f"world: hit-and-t-only records {share:.3f}")
            if share > kc.WORLD_T_ONLY_CAP:
                short.append(f"world: {share:.3f} of the records compare hit and t only (cap {kc.WORLD_T_ONLY_CAP})")
    print("\n".join(report))
    assert not short, "classes with fewer records than required, or a hit fraction outside [0.25, 0.75]: " + "; ".join(short)
