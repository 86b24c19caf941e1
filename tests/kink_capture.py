"""Reading the HIP path's kinks from the test side.

Every kink decision of the HIP backward pass is a function of an activation buffer the forward pass stored (tg_actgrad*, tg_mobn_bwd,
tg_bn_train_bwd_act and the column statistics read y; the pool backward kernels re-derive the arg-max from the pre-pool y).  Capture wraps
`new_act` of ONE live Context for the duration of a `with` block and logs every Act allocated inside, in call-site order; snapshot() copies
their logical [n,h,w,c] parts (no channel padding) to the host; match() finds, for every kink site of the oracle, the logged buffer that
holds the same tensor.  Nothing is patched at import and the class is left alone: the wrapper is an attribute of the instance and is
removed on exit."""
import numpy as np


class Capture(object):
    def __init__(self, cx):
        self.cx, self.log = cx, []

    def __enter__(self):
        orig = self.cx.new_act                    # the bound method of the class

        def new_act(*a, **kw):
            act = orig(*a, **kw)
            self.log.append(act)
            return act
        self.cx.new_act = new_act
        return self

    def __exit__(self, *exc):
        del self.cx.new_act
        return False

    def add(self, act):
        """log a handle a layer returned that new_act did not allocate (a view onto a concatenated buffer)."""
        self.log.append(act)
        return act

    def snapshot(self, upto=None):
        """host copies of the first `upto` logged float32 buffers (None for a handle without float32 storage)."""
        import torch
        torch.cuda.synchronize()
        return [a.numpy().copy() if (a.t is not None and a.dtype == 'f32') else None for a in self.log[:upto]]


def match(sites, arrays, act_tol, rows=None):
    """sites: forward-ordered (key, kind, y) with y the oracle's tensor over ALL rows of the batched call (kink_reference.cat_sites) or,
    with rows = (first image, images, images of the batched call), over ONE application's images, which are then cut out of the logged
    arrays (image-major in every layout).  For each site, the first logged array at or after the previous site's that has the element
    count and whose values agree with y within act_tol of max|y|.  A site without a match is a failure: nothing may stay un-injected.
    Returns ({key: array shaped like y}, {key: log index})."""
    out, where, pos = {}, {}, 0
    r0, n, total = rows if rows is not None else (0, 1, 1)
    for key, kind, y in sites:
        scale, best = np.abs(y).max(), None
        for j in range(pos, len(arrays)):
            a = arrays[j]
            if a is None or a.size * n != y.size * total:         # same elements in the same order (a dense layer's [n, h*w*c] output is its [n,h,w,c] view)
                continue
            a = a.reshape(total, -1)[r0:r0 + n]
            err = np.abs(a.reshape(y.shape) - y).max() / scale
            if err <= act_tol:
                out[key], where[key], pos = a.reshape(y.shape), j, j
                break
            best = err if best is None else min(best, err)
        assert key in out, ('oracle kink site without a logged activation that holds it', key, kind, y.shape, 'closest candidate', best,
                            [None if a is None else a.shape for a in arrays])
    return out, where
