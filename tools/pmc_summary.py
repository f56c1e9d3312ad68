"""Per-kernel medians of the counters in rocprofv3 `*_counter_collection.csv` files (--pmc passes).
Usage: python tools/pmc_summary.py <dir or csv> [kernel-name substring ...]   -> CSV on stdout

Behind the counters' own rows come the rows derived from them, per kernel, where the counters they need were collected
(in any of the files: one counter group per run, the runs side by side under <dir>):
  beyond_L2_GB      2 x FETCH_SIZE (KB) per launch: the bytes the L2s fetched from beyond them (on gfx950 FETCH_SIZE
                    reports half the bytes of wide reads: profiles/pmc_traffic.json); min and max are the launches' own
                    spread, what a change has to exceed
  written_GB        WRITE_SIZE (KB) per launch
  L2_hit_share      TCC_HIT_sum / (TCC_HIT_sum + TCC_MISS_sum), launch by launch
  effective_GHz     GRBM_GUI_ACTIVE / 8 XCDs / the launch's duration in that same run"""
import csv
import glob
import os
import statistics
import sys


def derived(vals, short):
  """[(row name, per-launch values, per-launch durations)] of one kernel from its counters' per-launch lists."""
  def col(name):
    return vals.get((short, name))
  out = []
  fetch, write, hit, miss, active = (col(n) for n in ('FETCH_SIZE', 'WRITE_SIZE', 'TCC_HIT_sum', 'TCC_MISS_sum',
                                                      'GRBM_GUI_ACTIVE'))
  if fetch:
    out.append(('beyond_L2_GB', [2.0 * x[0] * 1024 / 1e9 for x in fetch], [x[1] for x in fetch]))
  if write:
    out.append(('written_GB', [x[0] * 1024 / 1e9 for x in write], [x[1] for x in write]))
  if hit and miss and len(hit) == len(miss):
    out.append(('L2_hit_share', [h[0] / (h[0] + m[0]) if h[0] + m[0] else 0.0 for h, m in zip(hit, miss)],
                [x[1] for x in hit]))
  if active:
    out.append(('effective_GHz', [x[0] / 8.0 / x[1] if x[1] else 0.0 for x in active], [x[1] for x in active]))
  return out


def main(argv):
  src = argv[1]
  pats = argv[2:]
  files = [src] if os.path.isfile(src) else sorted(glob.glob(os.path.join(src, '**', '*counter_collection.csv'), recursive=True))
  vals = {}
  for f in files:
    for row in csv.DictReader(open(f)):
      name = row['Kernel_Name']
      if pats and not any(p in name for p in pats):
        continue
      short = name.replace('(anonymous namespace)::', '').split('(')[0][-90:]
      key = (short, row['Counter_Name'])
      vals.setdefault(key, []).append((float(row['Counter_Value']), int(row['End_Timestamp']) - int(row['Start_Timestamp']),
                                       row['VGPR_Count'], row['LDS_Block_Size']))
  print('"Kernel","Counter","Launches","MedianValue","MedianDurationNs","VGPRs","LDS_Block_Size","MinValue","MaxValue"')
  for (short, ctr), v in sorted(vals.items()):
    print('"%s","%s",%d,%.1f,%d,%s,%s,%.1f,%.1f' % (short, ctr, len(v), statistics.median(x[0] for x in v),
                                                    statistics.median(x[1] for x in v), v[0][2], v[0][3],
                                                    min(x[0] for x in v), max(x[0] for x in v)))
  for short in sorted(set(k[0] for k in vals)):
    first = next(v for k, v in vals.items() if k[0] == short)[0]
    for name, xs, durs in derived(vals, short):
      print('"%s","%s",%d,%.4f,%d,%s,%s,%.4f,%.4f' % (short, name, len(xs), statistics.median(xs), statistics.median(durs),
                                                      first[2], first[3], min(xs), max(xs)))


if __name__ == '__main__':
  main(sys.argv)
