#!/usr/bin/env python3
"""Every host path of the assemblies once, at small size, for a launch-by-launch comparison of two builds of the library whose device
code is the same (tools/unit_kernels.py) and whose host code differs: run it under `rocprofv3 --kernel-trace --output-format csv -d DIR --
python3 tools/launch_paths.py` in the tree of either build, then `launch_paths.py compare OLD_kernel_trace.csv NEW_kernel_trace.csv`.
compare: the multiset of (kernel name, grid, workgroup, LDS bytes) and the order of the launches within every queue must be equal;
it prints both totals and exits 1 on a difference.

Paths: dense 2D P1 with and without zero exterior, dense 2D P2, 1D, three order classes (label blocks off: one
context), a non-symmetric class table, a row slab, the H2 near field (cluster tiles), finite-horizon getSparse with and without
PNL_FH_NOTILES, pointwise dense and pointwise near field.  Several of them run on one context one after the other."""
import collections
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from pynucleus_amd import _lib, clusters, disc, interval, uniformSquare, PHYSICAL, dofmapFactory, getFractionalKernel
    from pynucleus_amd.builder import nonlocalBuilder
    from pynucleus_amd.fractionalOrders import layersFractionalOrder, smoothedLeftRightFractionalOrder
    from pynucleus_amd.linear_operators import DistributedSlab_LinearOperator
    torch.cuda.set_device(0)
    done = []

    def builder(mesh, order, element='P1', zeroExterior=True, **kw):
        dm = dofmapFactory(element, mesh, PHYSICAL)
        params = dict({'target_order': 0.5}, **kw.pop('params', {}))
        return nonlocalBuilder(dm, getFractionalKernel(mesh.dim, order, **kw), params, zeroExterior=zeroExterior)

    def path(name, fn):
        fn()
        torch.cuda.synchronize()
        done.append(name)
        print('path', name, flush=True)

    def near(b):
        rp = b.getH2RefinementParams()
        return clusters.getNearFieldClusters(b.dm, rp['eta'], rp['minSize'], rp['maxLevels'])[1]

    # one context: dense with settled tiles, the near field of cluster tiles, dense again
    b = builder(disc(5), 0.5)
    path('dense 2D P1, zero exterior', b.getDense)
    path('H2 near field (cluster tiles)', lambda: b.assembleClusters(near(b), forceUnsymmetricMatrix=True))
    path('dense 2D P1 after the near field', b.getDense)
    path('row slab', lambda: DistributedSlab_LinearOperator.assemble(b, 0, 2, None))
    path('dense 2D P1, no zero exterior', builder(disc(4), 0.4, zeroExterior=False).getDense)
    path('dense 2D P2', builder(disc(3), 0.5, element='P2').getDense)
    path('dense 1D', builder(interval(7), 0.75).getDense)
    # three order classes, then their near field (masked pairs, boundary items per class) on the same context
    layers = layersFractionalOrder(2, np.array([-1., 0., 1.]), np.array([[0.3, 0.5], [0.5, 0.7]]))
    b3 = builder(uniformSquare(17, None, -1., -1., 1., 1.), layers, params={'labelBlocks': False})
    path('dense, three order classes', b3.getDense)
    path('masked pairs, three order classes', lambda: b3.assembleClusters(near(b3)))
    ns = layersFractionalOrder(2, np.array([-1., -0.5, 0., 1.]), np.array([[0.3, 0.45, 0.5], [0.35, 0.5, 0.65], [0.6, 0.55, 0.7]]))
    bn = builder(uniformSquare(17, None, -1., -1., 1., 1.), ns, params={'labelBlocks': False})
    path('dense, non-symmetric class table', bn.getDense)
    path('masked pairs, non-symmetric class table', lambda: bn.assembleClusters(near(bn)))
    bh = builder(disc(4), 0.4, zeroExterior=False, horizon=0.3)
    path('finite horizon getSparse', bh.getSparse)
    _lib.set_option('PNL_FH_NOTILES', 1)
    path('finite horizon getSparse, PNL_FH_NOTILES', bh.getSparse)
    _lib.set_option('PNL_FH_NOTILES', None)
    bp = builder(disc(3), smoothedLeftRightFractionalOrder(0.25, 0.75, r=0.3))
    path('pointwise dense', bp.getDense)
    path('pointwise near field', lambda: bp.assembleClusters(near(bp)))
    print('{} paths'.format(len(done)))


def launches(trace):
    out = collections.defaultdict(list)
    with open(trace) as f:
        for r in sorted(csv.DictReader(f), key=lambda r: int(r['Dispatch_Id'])):
            out[r['Queue_Id']].append((r['Kernel_Name'], tuple(int(r['Grid_Size_'+d]) for d in 'XYZ'),
                                       tuple(int(r['Workgroup_Size_'+d]) for d in 'XYZ'), int(r['LDS_Block_Size'])))
    return out


def compare(old, new):
    a, b = launches(old), launches(new)
    ca, cb = (collections.Counter(l for q in t.values() for l in q) for t in (a, b))
    na, nb = sum(ca.values()), sum(cb.values())
    print('launches: {} old, {} new, {} distinct (kernel, grid, workgroup, LDS) old, {} new'.format(na, nb, len(ca), len(cb)))
    bad = 0
    for l in sorted(set(ca) | set(cb)):
        if ca[l] != cb[l]:
            print('count differs: {} old, {} new: {}'.format(ca[l], cb[l], l))
            bad += 1
    # the runtime numbers the queues as it makes them: pair them by their sequences, which must be equal as a multiset
    sa, sb = (sorted(tuple(q) for q in t.values()) for t in (a, b))
    print('queues: {} old {}, {} new {}'.format(len(sa), [len(q) for q in sa], len(sb), [len(q) for q in sb]))
    if sa != sb:
        print('the order of the launches within a queue differs')
        bad += 1
    print('equal' if not bad else 'DIFFERENT')
    return 1 if bad else 0


if __name__ == '__main__':
    if len(sys.argv) == 4 and sys.argv[1] == 'compare':
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    run()
