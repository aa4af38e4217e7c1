#!/usr/bin/env python3
"""rocprofv3 --pmc passes over tools/kbench.py -> counters PER DISPATCH of one kernel, per layer.

    python tools/pmc_kernels.py <manifest.json> <out.json> <build label> <kernel pattern> <layer regex> <counter_collection.csv> [more .csv ...]

Every csv is one rocprofv3 run of its own (counters only, no tracing) over the same kbench command; each holds a few
counters.  The trace is cut at the `af_marker_kernel` dispatches kbench puts in front of every timed op, segment k belongs to
entry k of kbench's manifest (which names the layer), and within a segment the counters of the dispatches whose kernel name
contains the pattern are averaged per instantiation.  The segments of a layer (kbench times it three times) are pooled; only
layers whose key `name|shape` matches the regex are written.
"""
import csv
import json
import re
import sys
from collections import defaultdict


def short_name(name):
    m = re.search(r'(\w+<[^>]*>|\w+)\s*\(', name.replace('(anonymous namespace)::', ''))
    return m.group(1) if m else name


def per_segment(path, pattern):
    """-> list over segments of {kernel: {'_n': dispatches, counter: sum}}"""
    csv.field_size_limit(1 << 30)
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Dispatch_Id']))
    segs, cur, marks = [], None, set()
    seen = set()
    for r in rows:
        name, did = r['Kernel_Name'], int(r['Dispatch_Id'])
        if 'af_marker_kernel' in name:
            if did not in marks:
                marks.add(did)
                cur = defaultdict(lambda: defaultdict(float))
                segs.append(cur)
            continue
        if cur is None or pattern not in name:
            continue
        k = cur[short_name(name)]
        k[r['Counter_Name']] += float(r['Counter_Value'])
        if did not in seen:
            seen.add(did)
            k['_n'] += 1
            k['_grid'] = float(r.get('Grid_Size', 0) or 0)
    return segs


def main():
    manifest, out, label, pattern, layers = json.load(open(sys.argv[1])), sys.argv[2], sys.argv[3], sys.argv[4], re.compile(sys.argv[5])
    pooled = defaultdict(lambda: defaultdict(lambda: defaultdict(float)))  # layer -> kernel -> counter -> sum
    counts = defaultdict(lambda: defaultdict(lambda: defaultdict(float)))  # layer -> kernel -> counter -> dispatches
    for path in sys.argv[6:]:
        segs = per_segment(path, pattern)
        assert len(segs) == len(manifest), (path, len(segs), len(manifest))
        for m, seg in zip(manifest, segs):
            if not m.get('name') or not m.get('shape'):
                continue
            layer = '%s|%s' % (m['name'], 'x'.join(str(v) for v in m['shape']))
            if not layers.search(layer):
                continue
            for kernel, c in seg.items():
                for counter, v in c.items():
                    if counter == '_n':
                        continue
                    if counter == '_grid':
                        pooled[layer][kernel]['_grid'] = v
                        continue
                    pooled[layer][kernel][counter] += v
                    counts[layer][kernel][counter] += c['_n']
    res = {'_meta': {'build': label, 'layers': layers.pattern, 'what': 'rocprofv3 --pmc alone (no tracing), one run per counter group, over tools/kbench.py; mean per '
                                              'dispatch of kernels matching %r, per kbench layer (the warm-up and the timed calls pooled)' % pattern}}
    for layer in pooled:
        res[layer] = {}
        for kernel, c in pooled[layer].items():
            res[layer][kernel] = {k: (v if k == '_grid' else v / counts[layer][kernel][k]) for k, v in c.items()}
            res[layer][kernel]['_dispatches'] = max(counts[layer][kernel].values())
    json.dump(res, open(out, 'w'), indent=1, sort_keys=True)
    print('wrote', out, len(res) - 1, 'layers')


if __name__ == '__main__':
    main()
