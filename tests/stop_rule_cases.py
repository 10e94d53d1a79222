"""Shared by tests/test_stop_rule_emu.py and tests/test_stop_rule_gpu.py: the inputs of the kernel cases, a numpy restatement of
lfsd_stop_compact / lfsd_gather_rows / lfsd_scatter_rows, and the reference's learning loop (lib/QuadAlgorithm.py:239-257) around a
batch-of-one learner WITHOUT a stop rule -- the yardstick of the learner cases."""
import numpy as np
import torch

LOSS_TOL = 0.9            # the reference's thresholds are 0.9 / 0.05; 0.0625 has an exact square and root, so a row can sit ON it
GRAD_TOL = 0.0625
ROW_COUNTS = (1, 63, 64, 65, 1023, 1025, 4099)
SENTINEL = -7


def norm_in(dt, g):
    """||g||_2 per row with every operation rounded to `dt`, summed in index order (what the kernel does, up to the contraction
    of a multiply-add: a few ulp, which stop_case keeps away from the threshold)."""
    s = np.zeros(g.shape[0], dtype=dt)
    for j in range(g.shape[1]):
        s = (s + g[:, j] * g[:, j]).astype(dt)
    return np.sqrt(s).astype(dt)


def stop_case(n_rows, dt, given, seed=0, n_param=7):
    """loss, grad (numpy, dtype dt), rows_in / eligible (or None), the size of the full batch.  Rows 0.. carry the special values:
    NaN loss, NaN gradient entry, Inf gradient entry, loss ON the threshold, norm ON the threshold (neither is 'greater')."""
    rng = np.random.RandomState(1000 * n_rows + seed + (7 if given else 0))
    loss = rng.uniform(0.0, 2.0, n_rows).astype(dt)
    grad = (rng.standard_normal((n_rows, n_param)) * 10.0 ** rng.uniform(-3.0, 0.0, (n_rows, 1))).astype(dt)
    # no norm within 4 ulp of the threshold (a contracted multiply-add may move it by one or two)
    nrm = norm_in(dt, grad)
    close = np.abs(nrm - dt(GRAD_TOL)) <= 4 * np.spacing(dt(GRAD_TOL))
    grad[close] *= dt(1.5)
    assert not (np.abs(norm_in(dt, grad) - dt(GRAD_TOL)) <= 4 * np.spacing(dt(GRAD_TOL))).any()
    special = []
    k = 0

    def put(l, g):
        nonlocal k
        if k < n_rows:
            if l is not None:
                loss[k] = l
            if g is not None:
                grad[k] = g
            special.append(k)
            k += 1
    big = np.full(n_param, 1.0, dtype=dt)
    put(np.nan, big)
    g = big.copy(); g[n_param // 2] = np.nan
    put(2.0, g)
    g = big.copy(); g[-1] = np.inf
    put(2.0, g)                                           # Inf norm > tol: goes on
    put(LOSS_TOL, big)                                    # loss == threshold (in dt): stops
    g = np.zeros(n_param, dtype=dt); g[1] = GRAD_TOL
    put(2.0, g)                                           # norm == threshold exactly: stops
    put(np.inf, big)                                      # Inf loss: goes on
    rows_in = eligible = None
    full = n_rows
    if given:
        full = n_rows + 37
        rows_in = np.sort(rng.choice(full, n_rows, replace=False)).astype(np.int32)
        eligible = (rng.uniform(size=n_rows) > 0.2).astype(np.int32)
        if n_rows > 1:
            eligible[1] = 0                               # an ineligible row with a NaN gradient is kept all the same
    return loss, grad, rows_in, eligible, full


def stop_reference(dt, loss, grad, rows_in, eligible, full, iter_idx, active0, stop_iter0):
    """numpy restatement: (rows_out, pos_out, n_out, active, stop_iter)."""
    n = loss.shape[0]
    with np.errstate(invalid="ignore", over="ignore"):
        keep = (loss > dt(LOSS_TOL)) & (norm_in(dt, grad) > dt(GRAD_TOL))
    if eligible is not None:
        keep = keep | (eligible == 0)
    orig = np.arange(n, dtype=np.int32) if rows_in is None else rows_in
    pos = np.nonzero(keep)[0].astype(np.int32)
    active, stop_iter = active0.copy(), stop_iter0.copy()
    active[orig[~keep]] = 0
    stop_iter[orig[~keep]] = iter_idx + 1
    return orig[pos], pos, len(pos), active, stop_iter


def run_stop_compact(lib, device, dt, n_rows, given, iter_idx=4):
    """One kernel case through ModelLibrary.stop_compact on `device`; asserts every integer output against the restatement."""
    loss, grad, rows_in, eligible, full = stop_case(n_rows, dt, given)
    rng = np.random.RandomState(n_rows)
    active0 = np.ones(full, dtype=np.int32)
    stop0 = np.zeros(full, dtype=np.int32)
    if given:                                            # rows that are not in the list stopped earlier: must stay as they are
        out = np.setdiff1d(np.arange(full), rows_in)
        active0[out] = 0
        stop0[out] = rng.randint(1, 4, len(out))
    t = lambda a: None if a is None else torch.from_numpy(a).to(device)
    rows_out = torch.full((n_rows,), SENTINEL, dtype=torch.int32, device=device)
    pos_out = torch.full((n_rows,), SENTINEL, dtype=torch.int32, device=device)
    n_out = torch.full((1,), SENTINEL, dtype=torch.int32, device=device)
    active, stop_iter = t(active0.copy()), t(stop0.copy())
    lib.stop_compact(t(loss), t(grad), LOSS_TOL, GRAD_TOL, iter_idx, rows_out, pos_out, n_out, active, stop_iter,
                     rows_in=t(rows_in), eligible=t(eligible))
    r_rows, r_pos, r_n, r_active, r_stop = stop_reference(dt, loss, grad, rows_in, eligible, full, iter_idx, active0, stop0)
    assert int(n_out.item()) == r_n
    assert np.array_equal(rows_out.cpu().numpy()[:r_n], r_rows) and np.array_equal(pos_out.cpu().numpy()[:r_n], r_pos)
    assert (rows_out.cpu().numpy()[r_n:] == SENTINEL).all() and (pos_out.cpu().numpy()[r_n:] == SENTINEL).all()
    assert np.array_equal(active.cpu().numpy(), r_active) and np.array_equal(stop_iter.cpu().numpy(), r_stop)
    assert 0 < r_n < n_rows or n_rows < 8                # (the case exercises both outcomes)
    return r_n


def run_row_copies(lib, device, n_rows, row_words, word=torch.int32, misalign=False):
    """lfsd_gather_rows and lfsd_scatter_rows on rows of `row_words` words of random BITS (NaN patterns included), against numpy
    indexing, bit for bit.  misalign: the dense side starts one word into its allocation (no 16-byte accesses possible)."""
    rng = np.random.RandomState(n_rows * 131 + row_words)
    full = n_rows + 29
    info = torch.iinfo(word)
    src_np = rng.randint(info.min, info.max, size=(full, row_words), dtype=np.int64).astype(np.int64)
    src = torch.from_numpy(src_np).to(word).to(device)
    index_np = rng.permutation(full)[:n_rows].astype(np.int32)
    index = torch.from_numpy(index_np).to(device)

    def dense(rows):
        flat = torch.full((rows * row_words + 1,), SENTINEL, dtype=word, device=device)
        return flat[1:].view(rows, row_words) if misalign else flat[:-1].view(rows, row_words)
    got = lib.gather_rows(index, src, dense(n_rows), n_rows)
    assert torch.equal(got.cpu(), src.cpu()[index_np.astype(np.int64)])
    back = torch.full((full, row_words), SENTINEL, dtype=word, device=device)
    lib.scatter_rows(index, got, back, n_rows)
    want = torch.full((full, row_words), SENTINEL, dtype=word)
    want[index_np.astype(np.int64)] = src.cpu()[index_np.astype(np.int64)]
    assert torch.equal(back.cpu(), want)


def reference_loop(make_learner, K, loss_tol, grad_tol):
    """lib/QuadAlgorithm.py:239-257 around ONE seed: `make_learner()` returns a batch-of-one SparseDemoLearner without a stop
    rule.  Returns (stop_iter, losses [k], grads [k,p], thetas [k+1,p]); stop_iter 0 = still running after K iterations."""
    L = make_learner()
    thetas, losses, grads = [L.theta[0].cpu().numpy().copy()], [], []
    loss, diff_loss_norm = 100.0, 100.0
    stop_iter = 0
    for j in range(K):
        if (loss > loss_tol) and (diff_loss_norm > grad_tol):
            l, g = L.step()
            loss = l[0].item()
            diff_loss_norm = float(np.linalg.norm(g[0].cpu().numpy()))
            losses.append(l[0].item()); grads.append(g[0].cpu().numpy().copy()); thetas.append(L.theta[0].cpu().numpy().copy())
        else:
            stop_iter = j
            break
    else:
        if not ((loss > loss_tol) and (diff_loss_norm > grad_tol)):
            stop_iter = K                                 # (met its test in the last iteration: the loop would break at j = K)
    return stop_iter, np.array(losses), np.array(grads), np.array(thetas)


def widest_gap(values):
    """Threshold in the middle (geometric) of the widest relative gap of the positive values."""
    v = np.unique(np.asarray(values, dtype=np.float64).ravel())
    v = v[v > 0]
    r = v[1:] / v[:-1]
    i = int(np.argmax(r))
    return float(np.sqrt(v[i] * v[i + 1]))
