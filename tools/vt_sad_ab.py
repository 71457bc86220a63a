#!/usr/bin/env python3
"""A/B timing of the true-SAD scan of uint8 view templates (GPU box).

usage: python tools/vt_sad_ab.py [--rounds 5] [--out profiles/vt_sad/vt_sad_ab.json]
One process.  For 1,000 and 10,000 templates of 64 x 32 and 1,024 queries (stored views rolled
by -7..7 rows with two-sided noise, one in ten a fresh image), three legs make the same
frozen call, match_templates(queries, mode=RS_VT_FROZEN), over the same bytes:
  float   the only true-SAD route before the metric: the float32-resident library
          (rs_vtf_scan) on the bytes cast to float32;
  sad     the uint8 library with metric='sad' (vt_scan_sad_kernel);
  plane   the uint8 library with the default wrapped metric (the pruned plane scan), for
          context only: another metric, whose pruning depends on the data.
Each leg is warmed up, then the legs alternate over the rounds.  Kernel time is the
library's own (rs_vt_last_ms / rs_vtf_last_ms: HIP events round the scan); per leg the
median over all timed calls and the spread, max - min of the per-round medians.
Acceptance: float's median exceeds sad's by more than the two spreads together, at both
sizes.  The sad leg's rate is also given as a fraction of the v_sad_u8 ceiling of the
issue-slot model in DESIGN.md (half-rate v_sad_u8, (H - 16) * W / 4 * 15 of them a compare).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, NQ = 64, 32, 1024
SIZES = (1000, 10000)
CALLS = {'float': 2, 'sad': 20, 'plane': 20}      # timed calls per leg and round
# 256 CUs x 4 SIMDs x 2.4 GHz / 2 cycles a wave instruction, v_sad_u8 at half of that, 64 lanes
SAD_PER_COMPARE = (H - 16) * (W // 4) * 15
CEILING = 256 * 4 * 2.4e9 / 2 * 0.5 * 64 / SAD_PER_COMPARE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sizes', default=','.join(str(s) for s in SIZES))
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vt_sad', 'vt_sad_ab.json'))
    ap.add_argument('--legs', default='float,sad,plane',
                    help='the legs to run (acceptance needs float and sad)')
    ap.add_argument('--lib', help='another build of the library (tools/build_variant.py), by path')
    a = ap.parse_args()
    legs = a.legs.split(',')
    import numpy as np
    from pyratslam_amd import _lib
    if a.lib:
        _lib.load(os.path.abspath(a.lib))
    from pyratslam_amd.view_templates import ViewTemplates
    results = []
    for T in (int(s) for s in a.sizes.split(',')):
        rng = np.random.default_rng(T)
        data = rng.integers(0, 256, (T, H, W), dtype=np.uint8)
        q = np.empty((NQ, H, W), np.uint8)
        for i in range(NQ):
            if i % 10:
                b = np.roll(data[int(rng.integers(0, T))], int(rng.integers(-7, 8)), axis=0)
                q[i] = np.clip(b.astype(np.int64) + rng.integers(-3, 4, (H, W)), 0, 255)
            else:
                q[i] = rng.integers(0, 256, (H, W), dtype=np.uint8)
        qf = q.astype(np.float32)
        libs = {k: ViewTemplates._from_shape((H, W), np.inf, capacity=T, metric='sad' if k == 'sad' else 'wrapped')
                for k in legs}
        for k, v in libs.items():
            v.add(data.astype(np.float32) if k == 'float' else data)
        forms = {k: v.scan_form() for k, v in libs.items()}
        want = {'float': 'sad-resident', 'sad': 'sad'}
        assert all(forms[k] == want.get(k, forms[k]) for k in legs), forms
        for v in libs.values():
            v.set_timing(True)
        got = {}

        def call(k):
            idx, score, _ = libs[k].match_templates(qf if k == 'float' else q, mode=_lib.RS_VT_FROZEN)
            got[k] = (idx, score)
            return libs[k].device_ms()

        for k in libs:                                   # warm-up of each leg
            for _ in range(2):
                call(k)
        # the two true-SAD routes agree on every query (every score < 2^24: exact in float32)
        if 'float' in got and 'sad' in got:
            assert np.array_equal(got['float'][0], got['sad'][0])
            assert np.array_equal(got['float'][1].astype(np.uint64), got['sad'][1])
        ms = {k: [] for k in libs}
        for _ in range(a.rounds):
            for k in libs:
                ms[k].append([call(k) for _ in range(CALLS[k])])
        row = {'templates': T, 'queries': NQ, 'shape': [H, W], 'rounds': a.rounds, 'forms': forms}
        for k, rows in ms.items():
            arr = np.array(rows)
            rm = np.median(arr, axis=1)
            med = float(np.median(arr))
            row[k] = {'median_ms': med, 'round_medians_ms': [float(x) for x in rm],
                      'spread_ms': float(rm.max() - rm.min()),
                      'gcompares_per_s': T * NQ / (med * 1e-3) / 1e9}
        f, s = row.get('float'), row.get('sad')
        if f and s:
            row['speedup_float_over_sad'] = f['median_ms'] / s['median_ms']
            row['accepted'] = bool(f['median_ms'] - s['median_ms'] > f['spread_ms'] + s['spread_ms'])
        if s:
            row['sad_fraction_of_ceiling'] = s['gcompares_per_s'] * 1e9 / CEILING
        if s and 'plane' in row:
            row['sad_over_plane'] = s['median_ms'] / row['plane']['median_ms']
        print(json.dumps(row), flush=True)
        results.append(row)
        for v in libs.values():
            v.close()
    out = {'ceiling_gcompares_per_s': CEILING / 1e9, 'sad_u8_per_compare': SAD_PER_COMPARE,
           'accepted': all(r.get('accepted', False) for r in results), 'sizes': results}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as fh:
        json.dump(out, fh, indent=1)
        fh.write('\n')
    return 0 if out['accepted'] else 1


if __name__ == '__main__':
    sys.exit(main())
