"""NumPy float64 restatement of tg_eval_report_f32 (include/tg_kernels.h, csrc/evalreport.hip), row by row, for
tests/test_eval_report_reference.py and tests/test_gpu_eval_report.py.  Not collected.

The arg-max is accuracy_kernel's scan written as the loop it is (`a = 0; for j: if row[j] > row[a]: a = j`), so ties, NaN and infinities
fall where the comparison puts them.  Everything an integer output counts is exact here; the three fp64 accumulations come with the
bound the GPU test holds the device to:

    bound = (k + n + 64) * 2^-52 * sum |terms|

one rounding per exact-difference conversion ((double)l_j - (double)m, (double)m - (double)l_t), at most 2 ulp for each of exp / log on
either side, k fp64 additions over the classes and then n over the rows.  `terms` are the quantities those relative errors act on:
  bin_conf[b]  the confidences conf = 1 / s of the bin's rows (s = sum_j e_j carries the relative error of its terms; so does 1 / s);
  sums[0]      per row |log s| + |m - l_t| + 1: the two terms that are added, and 1 = sum_j e_j / s for the sum under the logarithm, whose
               RELATIVE error the logarithm hands on as an ABSOLUTE one (d log s = ds / s) however small log s itself is (a confident,
               correct row has log s ~ 1e-9 and an NLL to match);
  sums[1]      per row sum_j (p_j + y_j)^2: (p_j - y_j)^2 = p_j^2 - 2 p_j y_j + y_j^2 with every term taken absolutely — p_t - 1 cancels
               for a confident correct row, and the error of p_t does not shrink with the difference.
Both per-row magnitudes are >= 1, so neither bound collapses on a batch of saturated rows."""
import numpy as np

EPS = 2.0 ** -52


def scan_argmax(row):
    """accuracy_kernel's arg-max (csrc/loss.hip): start at 0, move to j only on strictly greater."""
    a = 0
    for j in range(1, len(row)):
        if row[j] > row[a]:
            a = j
    return a


def reference(logits, labels, k, nr, nb):
    """logits [n, ld >= k], labels [n, ld_y >= k] float32 host arrays (columns k.. are not looked at) -> dict of
      confusion [k, k], rank_hist [nr], bin_count [nb], bin_correct [nb], nonfinite [1]   int64, exact
      bin_conf [nb], sums [2]                                                             float64
      bound_bin_conf [nb], bound_sums [2]     the bound of the module docstring for each fp64 output
      t, p [n] int; finite [n] bool; rank [n] int (-1: non-finite row); conf, nll, brier [n] float64 (NaN: non-finite row); bin [n] int (-1)
      bin_distance [n]    |conf * nb - nearest integer| (NaN: non-finite row): how far the row is from changing its bin."""
    logits, labels = np.asarray(logits, np.float32), np.asarray(labels, np.float32)
    n = logits.shape[0]
    out = dict(confusion=np.zeros((k, k), np.int64), rank_hist=np.zeros(nr, np.int64), bin_count=np.zeros(nb, np.int64),
               bin_correct=np.zeros(nb, np.int64), nonfinite=np.zeros(1, np.int64), bin_conf=np.zeros(nb), sums=np.zeros(2),
               t=np.zeros(n, np.int64), p=np.zeros(n, np.int64), finite=np.zeros(n, bool), rank=np.full(n, -1, np.int64),
               conf=np.full(n, np.nan), nll=np.full(n, np.nan), brier=np.full(n, np.nan), bin=np.full(n, -1, np.int64),
               bin_distance=np.full(n, np.nan))
    abs_conf, abs_sums = np.zeros(nb), np.zeros(2)
    for r in range(n):
        l32, y32 = logits[r, :k], labels[r, :k]
        t, p = scan_argmax(y32), scan_argmax(l32)
        out['t'][r], out['p'][r] = t, p
        out['confusion'][t, p] += 1
        if not np.isfinite(l32).all():
            out['nonfinite'][0] += 1
            continue
        out['finite'][r] = True
        rank = int((l32 > l32[t]).sum() + (l32[:t] == l32[t]).sum())
        out['rank'][r] = rank
        out['rank_hist'][min(rank, nr - 1)] += 1
        l = l32.astype(np.float64)
        m = l[p]
        e = np.exp(l - m)
        s = e.sum()
        conf = 1.0 / s
        nll = np.log(s) + (m - l[t])
        y = np.zeros(k)
        y[t] = 1.0
        pj = e / s
        brier = ((pj - y) ** 2).sum()
        x = conf * nb
        b = min(nb - 1, int(x))
        out['conf'][r], out['nll'][r], out['brier'][r], out['bin'][r], out['bin_distance'][r] = conf, nll, brier, b, abs(x - np.rint(x))
        out['bin_count'][b] += 1
        out['bin_correct'][b] += int(p == t)
        out['bin_conf'][b] += conf
        out['sums'] += (nll, brier)
        abs_conf[b] += conf
        abs_sums += (abs(np.log(s)) + abs(m - l[t]) + 1.0, ((pj + y) ** 2).sum())
    out['bound_bin_conf'] = (k + n + 64) * EPS * abs_conf
    out['bound_sums'] = (k + n + 64) * EPS * abs_sums
    return out


COUNT_KEYS = ('confusion', 'rank_hist', 'bin_count', 'bin_correct', 'bin_conf', 'sums', 'nonfinite')


def counts(ref):
    """the arguments of tg.metrics.report_from_counts out of reference()'s dict."""
    return {key: ref[key] for key in COUNT_KEYS}
