#!/usr/bin/env python
"""Compare the arrays of three `bench.py --dump-outputs` directories: two runs of the parent build and one of the new build.

    python tools/dump_compare.py PARENT_A PARENT_B NEW

Per array: its scale (max |value| over the three), the largest difference of every pair relative to that scale, and whether
the arrays are bit-equal.  The new build computes what the parent computed when parent_a/new is no larger than
parent_a/parent_b is, up to the noise of the kernels that reduce in a varying order (bench.py's docstring)."""
import os
import sys

import numpy as np

a_dir, b_dir, n_dir = sys.argv[1:4]
names = sorted(f[:-4] for f in os.listdir(a_dir) if f.endswith('.npy'))
worst = {'flows': [0.0, 0.0, 0.0], 'grads': [0.0, 0.0, 0.0]}
for name in names:
    a, b, n = (np.load(os.path.join(d, name + '.npy')) for d in (a_dir, b_dir, n_dir))
    finite = bool(np.isfinite(a).all() and np.isfinite(b).all() and np.isfinite(n).all())
    if name == 'loss':
        print('loss parent_a %r parent_b %r new %r finite %s bit-equal a/b %s a/new %s' % (
            float(a.reshape(-1)[0]), float(b.reshape(-1)[0]), float(n.reshape(-1)[0]), finite, a.tobytes() == b.tobytes(), a.tobytes() == n.tobytes()))
        continue
    scale = max(float(np.abs(t).max()) for t in (a, b, n)) or 1.0
    d = [float(np.abs(p - q).max()) / scale for p, q in ((a, b), (a, n), (b, n))]
    key = 'grads' if name == 'grads' else 'flows'
    worst[key] = [max(w, v) for w, v in zip(worst[key], d)]
    print('%-12s scale %e  parent_a/parent_b %.3e  parent_a/new %.3e  parent_b/new %.3e  equal a/b %s a/new %s finite %s' % (
        name, scale, d[0], d[1], d[2], a.tobytes() == b.tobytes(), a.tobytes() == n.tobytes(), finite))
for key in ('flows', 'grads'):
    print('WORST %s: parent_a/parent_b %.3e  parent_a/new %.3e  parent_b/new %.3e' % ((key,) + tuple(worst[key])))
