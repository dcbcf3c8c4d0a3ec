"""Drop-in replacement for the reference's `defences` module (reference defences.py:1-75).

Same names, same call signatures, same return conventions; the arithmetic runs in libbyzagg's HIP kernels
on an MI355X.  `Server.defend` (reference server.py:87) calls

    defences.defend[defence_method](self.users_grads, len(self.users), int(len(self.users)*self.mal_prop))

with a C-contiguous np.float32 matrix and gets a 1-D np.float32 vector back.  Device-resident inputs
(torch CUDA tensors) are accepted too and then nothing crosses PCIe.

Differences a caller can observe, all documented in DESIGN.md:
  * `krum` on a host numpy matrix returns a VIEW of the winning row, as the reference does (defences.py:42); on a
    device-resident matrix it returns a copy made on the device, so that the index need not cross to the host;
  * `_krum_create_distances` returns a `Distances` handle (GPU-resident N x N matrix) instead of a dict
    of dicts; `krum(..., distances=handle)` accepts it, `handle.to_dict()` rebuilds the reference's form.
"""
import numpy as np

from .engine import (DeviceBuffer, Distances, bucketing_permutation, dnc_columns, get_engine,  # noqa: F401
                     signguard_sample, signguard_window)


class DefenseTypes:
    NoDefense = 'NoDefense'
    Krum = 'Krum'
    TrimmedMean = 'TrimmedMean'
    Bulyan = 'Bulyan'

    def __str__(self):
        return self.value


def _upload_once(users_grads, stage=True):
    """(matrix, back): a host matrix uploaded once for the calls that follow (stage=False: left where it is), and what brings
    a result of theirs back -- back(v) is v.numpy() for a DeviceBuffer when the matrix came from the host, else v."""
    matrix, host = get_engine().stage(users_grads) if stage else (users_grads, False)
    return matrix, (lambda v: v.numpy() if host and isinstance(v, DeviceBuffer) else v)


def no_defense(users_grads, users_count, corrupted_count):
    """Column mean of the gradient matrix (reference defences.py:13-14)."""
    return get_engine().no_defense(users_grads, users_count, corrupted_count)


def _krum_create_distances(users_grads):
    """All pairwise client distances (reference defences.py:16-21), kept on the GPU."""
    return get_engine().pairwise_distances(users_grads)


def krum(users_grads, users_count, corrupted_count, distances=None, return_index=False, debug=False):
    """Krum as the reference defines it (defences.py:23-42): unsquared norms, the n-f smallest summed,
    candidates visited in the order 1, 0, 2, ... with a strict '<'."""
    return get_engine().krum(users_grads, users_count, corrupted_count, distances=distances,
                             return_index=return_index)


def trimmed_mean(users_grads, users_count, corrupted_count):
    """Mean of the k = rows - corrupted - 1 values closest to the median, per parameter
    (reference defences.py:44-52)."""
    return get_engine().trimmed_mean(users_grads, users_count, corrupted_count)


def bulyan(users_grads, users_count, corrupted_count):
    """Bulyan (reference defences.py:55-70): n - 2f iterated Krum picks, then the trimmed mean of the picked
    rows in selection order."""
    return get_engine().bulyan(users_grads, users_count, corrupted_count)


def multi_krum(users_grads, users_count, corrupted_count, m=None, distances=None, return_index=False):
    """Multi-Krum (Blanchard et al. 2017, section 4; not in the reference): every client scored the Krum way (the
    reference's n - f smallest distances, so that m = 1 is Krum), the m best (default users_count - corrupted_count)
    averaged.  The mean is np.mean(users_grads[np.sort(selection)], axis=0).  `return_index=True` returns the selection,
    best first, instead (and, as `krum` does, skips the users_count >= 2*corrupted_count + 1 assertion).  Not one of the
    `defend` keys: the reference's main.py offers only those four."""
    engine = get_engine()
    if return_index:
        if distances is None:
            distances = engine.pairwise_distances(users_grads)
        return engine.multi_krum_select(distances, users_count, corrupted_count, m)
    return engine.multi_krum(users_grads, users_count, corrupted_count, m=m, distances=distances)


def geometric_median(users_grads, users_count, corrupted_count, nu=1e-6, max_iter=10, ftol=1e-6):
    """The geometric median of the clients' gradients (smoothed Weiszfeld iterations: RFA, Pillutla, Kakade and
    Harchaoui; not in the reference).  The reference's signature, so that it drops into Server.defend-style calls;
    users_count and corrupted_count are accepted and unused (the median needs no count).  nu, max_iter and ftol are this
    package's defaults.  Not one of the `defend` keys: the reference's main.py offers only those four."""
    return get_engine().geometric_median(users_grads, nu=nu, max_iter=max_iter, ftol=ftol)


def centered_clip(users_grads, users_count, corrupted_count, tau=10.0, iters=3, start=None):
    """Centered clipping (Karimireddy, He and Jaggi, ICML 2021, Algorithm 2; not in the reference): from `start` (None: the
    zero vector; the previous round's aggregate is the paper's choice) every client's vector is pulled towards the centre
    and no client moves it by more than tau / n per iteration.  start=None with iters=1 is the norm-clipped mean, the
    standard answer to the backdoor attack.  The reference's signature; users_count and corrupted_count are accepted and
    unused.  tau = 10.0 and iters = 3 are this package's choices.  Not one of the `defend` keys: the reference's main.py
    offers only those four."""
    return get_engine().centered_clip(users_grads, tau=tau, iters=iters, start=start)


def fltrust(users_grads, users_count, corrupted_count, root_grad, return_info=False):
    """FLTrust (Cao, Fang, Liu and Gong, NDSS 2021; not in the reference): every client's vector is scored by the ReLU of its
    cosine with `root_grad`, the gradient the server computed on its own small root dataset, rescaled to that gradient's
    norm, and the scores weight the mean.  The one rule here that needs no honest majority: a vector pointing away from the
    root gets no weight however many agree with it.  No trusted client, or a zero or non-finite root: the zero vector.  The
    reference's leading signature; users_count and corrupted_count are accepted and unused.  return_info=True also returns
    Engine.fltrust's info.  Not one of the `defend` keys: the reference's main.py offers only those four, and none of them
    takes a root gradient."""
    return get_engine().fltrust(users_grads, root_grad, return_info=return_info)


def signguard(users_grads, users_count, corrupted_count, frac=0.1, lower=0.1, upper=3.0, bandwidth=None, n_samples=50, seed=0,
              window=None, sample=None, return_info=False):
    """SignGuard (Xu, Huang, Song and Lan, "Byzantine-robust Federated Learning through Collaborative Malicious Gradient
    Filtering", ICDCS 2022; not in the reference): the clients whose norm is outside (lower, upper) x the median norm are
    filtered, the clients are clustered by mean shift on their shares of positive, zero and negative coordinates over a
    random window of the coordinates, and the mean of the largest cluster's surviving vectors, each clipped to the median
    norm, is returned.  It is built for the reference's own attack: an "A Little Is Enough" vector sits among the honest ones
    in distance, and its sign shares give it away.  No client kept: the zero vector.
    lower = 0.1 and upper = 3.0 are the paper's numbers.  The window of a tenth of the coordinates (frac), the bandwidth
    quantile 0.5 and the 50 sampled clients (n_samples) are the authors' code's.  This package's: the window's start is
    uniform in [0, D - m] with both ends included (the authors' upper end is exclusive and cannot express frac = 1), the
    window and the sample are drawn on the host from `seed` (signguard_window, signguard_sample) unless `window` =
    (start, length) or `sample` give them, and a bandwidth below 2^-20 counts as zero (one cluster).  The paper draws a new
    window every round: pass a new seed per round (DeviceServer.defend_signguard does).  The reference's leading signature;
    users_count and corrupted_count are accepted and unused.  return_info=True also returns Engine.signguard's info.  Not
    one of the `defend` keys: the reference's main.py offers only those four."""
    return get_engine().signguard(users_grads, frac=frac, lower=lower, upper=upper, bandwidth=bandwidth, n_samples=n_samples,
                                  seed=seed, window=window, sample=sample, return_info=return_info)


def nnm(users_grads, users_count, corrupted_count, then=None, distances=None, **then_kwargs):
    """Nearest-neighbour mixing (Allouah et al., "Fixing by Mixing", AISTATS 2023; not in the reference): every client's vector
    is replaced by the mean of its users_count - corrupted_count nearest neighbours, itself included -- np.mean(users_grads[
    list_i], axis=0) bit for bit, the list in ascending row order.  A pre-aggregation: with then=None the mixed n x D matrix
    comes back; with a callable the result is then(mixed, users_count, corrupted_count, **then_kwargs) -- `krum`,
    `trimmed_mean`, `coordinate_median`, `geometric_median`, ... -- and the mixed matrix stays on the device in between.
    `distances` (optional): a `Distances` handle of users_grads.  Not one of the `defend` keys: the reference's main.py offers
    only those four, and this is no rule by itself."""
    matrix, back = _upload_once(users_grads, stage=then is not None)
    mixed = get_engine().nnm(matrix, users_count, corrupted_count, distances=distances)
    return mixed if then is None else back(then(mixed, users_count, corrupted_count, **then_kwargs))


def bucketing(users_grads, users_count, corrupted_count, s=2, then=None, perm=None, seed=0, **then_kwargs):
    """s-bucketing (Karimireddy, He and Jaggi, "Byzantine-Robust Learning on Heterogeneous Datasets via Bucketing", ICLR 2022;
    not in the reference): the clients are shuffled and every s consecutive ones replaced by their mean --
    np.mean(users_grads[perm[b*s:(b+1)*s]], axis=0) bit for bit; the last bucket may be short.  s is the bucket size: larger
    buckets average more of the honest clients' heterogeneity away, and a bad client still spoils one bucket only, so at
    most corrupted_count of the ceil(rows / s) buckets are bad; the paper's experiments use s = 2, the default here.  A
    pre-aggregation: with then=None the bucketed ceil(rows / s) x D matrix comes back; with a callable the result is
    then(bucketed, ceil(rows / s), corrupted_count, **then_kwargs) -- `krum`, `coordinate_median` (median-of-means),
    `geometric_median`, `centered_clip`, ... -- with the corrupted count passed on unchanged, as the paper's bound has it
    (the rule's own assertions decide whether s was too large for it), and the bucketed matrix stays on the device in
    between; a host matrix is uploaded once and the answer comes back as numpy.  The shuffle is `perm` if given, else
    bucketing_permutation(rows, seed), drawn on the host; the paper reshuffles every round, so pass a new seed per round.
    Pre-aggregations chain: bucketing(..., then=functools.partial(nnm, then=rule)).  Not one of the `defend` keys: the
    reference's main.py offers only those four, and this is no rule by itself."""
    rows = int(users_grads.shape[0])
    if perm is None:
        perm = bucketing_permutation(rows, seed)
    matrix, back = _upload_once(users_grads, stage=then is not None)
    bucketed = get_engine().bucket_means(matrix, s, perm)
    return bucketed if then is None else back(then(bucketed, -(-rows // int(s)), corrupted_count, **then_kwargs))


def robust_lr(users_grads, users_count, corrupted_count, theta=None, then=None, return_votes=False, **then_kwargs):
    """The robust learning rate (Ozdayi, Kantarcioglu and Gel, AAAI 2021; not in the reference), the defence designed for the
    backdoor attack: per coordinate the clients' updates vote with their signs (votes = #positive - #negative; zeros and NaN
    abstain), and where abs(votes) < theta the aggregate's sign bit is inverted -- with server.py:89-90's update that is the
    paper's negated learning rate for that coordinate.  No rule by itself: it wraps an aggregate.  then=None wraps the plain
    mean (no_defense's bits), vote and mean in one read of the matrix; with a callable the aggregate is then(users_grads,
    users_count, corrupted_count, **then_kwargs) -- `trimmed_mean`, `coordinate_median`, `centered_clip`, ... -- on the
    device-resident matrix (a host matrix is uploaded once) and the vote is a walk of its own.  theta: an integer in
    [0, rows]; the default corrupted_count + 1 is the smallest threshold that corrupted_count colluding clients cannot reach
    on their own -- this package's choice, the paper fixes no formula.  return_votes=True returns (aggregate, votes): the
    int32 votes' sign is signSGD's majority vote.  Not one of the `defend` keys: the reference's main.py offers only those
    four."""
    engine = get_engine()
    if theta is None:
        theta = int(corrupted_count) + 1
    theta = engine._theta(theta, int(users_grads.shape[0]))
    if then is None:
        return engine.robust_lr(users_grads, theta, return_votes=return_votes)
    matrix, back = _upload_once(users_grads)
    agg = then(matrix, users_count, corrupted_count, **then_kwargs)
    votes = engine.sign_votes(matrix)
    out, votes = back(engine.sign_flip(agg, votes, theta)), back(votes)
    return (out, votes) if return_votes else out


def sparsefed(users_grads, users_count, corrupted_count, k=None, clip=10.0, residual=None, then=None, return_residual=False,
              **then_kwargs):
    """SparseFed (Panda, Mahloujifar, Bhagoji, Chakraborty and Mittal, AISTATS 2022; not in the reference), the other defence
    designed for model poisoning such as the backdoor attack: the aggregate is added to an error-feedback memory W and only
    the k coordinates of W with the largest magnitude are applied; the rest stay in W for later rounds.  then=None is the
    paper's rule -- every client clipped to norm `clip`, then the mean (centered_clip from zero with one iteration) -- and
    runs as ONE library call.  With a callable the aggregate is then(users_grads, users_count, corrupted_count,
    **then_kwargs) -- `coordinate_median`, `trimmed_mean`, ... -- on the device-resident matrix (a host matrix is uploaded
    once) and the top-k a call of its own; `clip` is then unused.  `residual` is the caller's memory W, updated IN PLACE when
    given (a writable float32 numpy vector for a host matrix, a device-resident one for a device matrix); None means a
    zero memory.  k: an integer in [0, D]; the default max(1, D // 100) is this package's choice, the paper fixes no
    formula.  The selection's order is total: magnitude by the bits (zeros tie, infinities above every finite value, NaN
    above them, nothing sanitised), ties to the lower column.  return_residual=True returns (step, residual).  Not one of
    the `defend` keys: the reference's main.py offers only those four."""
    engine = get_engine()
    d = int(users_grads.shape[1])
    if k is None:
        k = max(1, d // 100)
    k = engine._topk_k(k, d)
    if then is None:
        out, res = engine.sparsefed(users_grads, k, clip=clip, residual=residual)
        return (out, res) if return_residual else out
    if not callable(then):
        raise TypeError('sparsefed: `then` is the rule that supplies the aggregate, e.g. defences.coordinate_median, or None')
    matrix, back = _upload_once(users_grads)
    agg = then(matrix, users_count, corrupted_count, **then_kwargs)
    if residual is None:
        out, res = engine.topk_sparsify(agg, k)              # a zero memory: W is the aggregate
    else:
        out, res = engine.topk_sparsify(residual, k, add=agg, residual=residual)
    return (back(out), back(res)) if return_residual else back(out)


def gaussian_noise(vector, sigma, seed=0, round=0, column_offset=0):
    """vector + sigma * z: z the standard normals of the library's Philox4x32-10 stream (include/byzagg.h), drawn on the GPU and
    addressed by GLOBAL column -- column c of `vector` takes z[column_offset + c], so a slice of a longer vector with its
    offset gets exactly the noise the whole vector would.  One fp64 addition, rounded once to float32.  `round` is the
    caller's round counter: one seed, fresh noise every round.  numpy in -> numpy out; device-resident in ->
    device-resident out."""
    return get_engine().gaussian_noise(vector, sigma, seed=seed, round=round, column_offset=column_offset)


def weak_dp(users_grads, users_count, corrupted_count, clip=10.0, sigma=0.01, adaptive=False, seed=0, round=0, then=None,
            return_info=False, **then_kwargs):
    """Norm clipping plus Gaussian noise, "weak DP" (Sun, Kairouz, Suresh and McMahan 2019; not in the reference): the
    baseline the backdoor defences (robust_lr, sparsefed) measure themselves against, FLAME's last stage (Nguyen et al.
    2022) and DP-FedAvg's server step.  then=None runs as ONE library call: every client clipped to norm `clip`, the mean
    (centered_clip from zero with one iteration; a client with a non-finite entry is excluded and still counted), then
    gaussian_noise with standard deviation sigma.  adaptive=True is FLAME's: clip = the median of the clients' finite
    norms and the noise's standard deviation sigma * clip (sigma is then FLAME's lambda), nothing read by the host.  With a
    callable the noise goes on then(users_grads, users_count, corrupted_count, **then_kwargs) -- `coordinate_median`,
    `trimmed_mean`, ... -- on the device-resident matrix (a host matrix is uploaded once); `clip` is then unused and
    adaptive is refused.  clip = 10.0 and sigma = 0.01 are this package's choice: the papers tune both.  (seed, round)
    name the noise vector: the same pair gives the same vector, DeviceServer.defend_weak_dp counts the rounds.
    return_info=True returns (vector, {clipped_rows, excluded_rows, clip}) (then=None only).  Not one of the `defend` keys:
    the reference's main.py offers only those four."""
    engine = get_engine()
    if then is None:
        return engine.weak_dp(users_grads, clip=clip, sigma=sigma, adaptive=adaptive, seed=seed, round=round,
                              return_info=return_info)
    if not callable(then):
        raise TypeError('weak_dp: `then` is the rule that supplies the aggregate, e.g. defences.coordinate_median, or None')
    if adaptive or return_info:
        raise ValueError('weak_dp: adaptive and return_info describe the clipping, which a rule `then` replaces')
    matrix, back = _upload_once(users_grads)
    return back(engine.gaussian_noise(then(matrix, users_count, corrupted_count, **then_kwargs), sigma, seed=seed, round=round))


def cosine_distances(users_grads):
    """The pairwise cosine distances of the clients' rows, 1 - cos, as a `Distances` handle resident on the GPU (diagonal
    +inf, a zero or non-finite client's row and column +inf): what `flame` clusters on, and what its `distances=` takes."""
    return get_engine().cosine_distances(users_grads)


def flame(users_grads, users_count, corrupted_count, lam=0.001, min_samples=1, min_cluster_size=None, seed=0, round=0,
          distances=None, return_info=False):
    """FLAME (Nguyen et al., USENIX Security 2022; not in the reference): the backdoor defence `robust_lr`, `sparsefed` and
    `weak_dp` are measured against.  Pairwise cosine distances between the clients; HDBSCAN with min_cluster_size =
    n // 2 + 1 and everything outside the one majority cluster rejected; the admitted clients clipped to the median norm of
    all clients and averaged; Gaussian noise of standard deviation lam * (that median) drawn on the GPU.  One library call,
    nothing read by the host.  By construction roughly half of the clients, the densest majority, are admitted; identical
    rows sit together at distance 0 and are admitted as a block, so this is a backdoor defence, not an answer to the drift
    attack.  Nobody admitted (too many zero or non-finite clients): the zero vector plus the noise.
    min_samples follows the `hdbscan` package's convention; scikit-learn's min_samples is one more.  lam = 0.001 is this
    package's default: the paper tunes it per task.  The paper compares the clients' local MODELS; this compares the rows
    it is given, and a caller who wants the models' angles passes them as `distances=` (a `Distances` handle, e.g.
    cosine_distances(models), or a dense matrix with an infinite diagonal), which replaces the cosine stage.  (seed, round)
    name the noise vector; DeviceServer.defend_flame counts the rounds.  The reference's leading signature; users_count
    and corrupted_count are accepted and unused.  numpy in -> numpy out, device-resident in -> device-resident out.
    return_info=True returns (vector, {admitted_rows, admitted, broken_rows, w_star, clip}).  Not one of the `defend` keys:
    the reference's main.py offers only those four."""
    return get_engine().flame(users_grads, lam=lam, min_samples=min_samples, min_cluster_size=min_cluster_size, seed=seed,
                              round=round, distances=distances, return_info=return_info)


def manhattan_distances(users_grads):
    """The pairwise Manhattan (L1) distances of the clients' rows as a `Distances` handle resident on the GPU (diagonal
    +inf, a pair whose sum is not finite +inf): what `multi_metrics` adds to the Euclidean and cosine matrices, and what
    `krum`, `multi_krum`, `nnm` and `flame` take as `distances=` to run on L1 geometry."""
    return get_engine().manhattan_distances(users_grads)


def multi_metrics(users_grads, users_count, corrupted_count, p=0.3, return_info=False):
    """Multi-Metrics (Huang et al., ICCV 2023; not in the reference): the backdoor defence beside `flame`, `robust_lr` and
    `sparsefed`.  Every client is described by its summed Manhattan, Euclidean and cosine distance to the other usable
    clients (a zero or non-finite client is not usable); the three features are divided by their standard deviations and
    scored by the squared Mahalanobis norm under their correlation matrix, uncentred, as in the paper; the int(p * n)
    clients of smallest score (ties to the lower row) are averaged: np.mean(users_grads[chosen], axis=0), bit for bit.
    Fewer than four usable clients, a constant feature or a singular correlation matrix: the Manhattan feature alone
    scores.  Nobody usable: the zero vector.  One library call, nothing read by the host.  p = 0.3 is the paper's; p > 1
    and int(p * n) < 1 are refused.  The reference's leading signature; users_count and corrupted_count are accepted and
    unused.  numpy in -> numpy out, device-resident in -> device-resident out.  return_info=True returns (vector,
    {chosen_rows, kept, usable, degenerate, det}).  Not one of the `defend` keys: the reference's main.py offers only those
    four."""
    return get_engine().multi_metrics(users_grads, p=p, return_info=return_info)


def linkage_labels(distances, n_clusters=2, method='average', fill=2.0):
    """Agglomerative clustering of a distance matrix (a `Distances` handle -- cosine_distances, _krum_create_distances,
    manhattan_distances -- or a dense symmetric matrix, the diagonal ignored) cut into `n_clusters`, on the GPU: int32 labels,
    the clusters numbered by their lowest row in ascending order, -1 for a row without a finite off-diagonal distance, which
    takes no part.  method: 'average', 'complete' or 'single'; an entry that is not finite or is negative counts as `fill`.
    Engine.linkage returns the whole dendrogram in scipy's format."""
    engine = get_engine()
    pair, _, _, usable = engine.linkage_merges(distances, method=method, fill=fill)
    return engine.linkage_cut(pair, usable, n_clusters)[0]


def clipped_clustering(users_grads, users_count, corrupted_count, clip=None, method='average', distances=None, norm_history=None,
                       max_tau=1e5, return_info=False):
    """ClippedClustering (Li, Ngai and Voigt, IEEE Trans. Big Data 2023; Blades' `Clippedclustering`; not in the reference):
    every client clipped to the median norm, pairwise cosine distances, agglomerative clustering with average linkage cut
    into two clusters, the mean of the larger one.  Scaling a row by a positive number does not change its cosines, so the
    cosine stage runs on the UNCLIPPED rows (Blades clips first: the same distances).  Distances that are not finite count
    as 2.0, the largest cosine distance, as in Blades; a zero or non-finite client takes no part.  Equal cluster sizes: the
    cluster of the lowest usable row is admitted (Blades' tie goes to scikit-learn's label 0, which is not a property of
    the data).  With two or more usable clients the two-way cut ALWAYS rejects somebody: the rule never returns the plain
    clipped mean.  One usable client: it alone; none: the zero vector.
    clip=None is the adaptive mode, the median of this round's finite norms: one library call, nothing read by the host.
    clip > 0 is a fixed threshold.  norm_history, a Python list, is the paper's running threshold (Blades' `l2norm_his`):
    the call appends this round's n norms to it IN PLACE and clips to min(np.median of its finite entries, max_tau); the
    norms are read back for that, which is ONE synchronisation, and are handed to the library so that it does not compute
    them again.  method: 'average' (the paper's), 'complete' or 'single'.  `distances=` (a `Distances` handle or a dense
    matrix) replaces the cosine stage.  The reference's leading signature; users_count and corrupted_count are accepted and
    unused.  numpy in -> numpy out, device-resident in -> device-resident out.  return_info=True returns (vector,
    {admitted_rows, admitted, usable, top_height, second_height, clip}).  Not one of the `defend` keys: the reference's
    main.py offers only those four."""
    engine = get_engine()
    if norm_history is None:
        return engine.clipped_clustering(users_grads, clip=clip, method=method, distances=distances, return_info=return_info)
    if clip is not None:
        raise ValueError('clipped_clustering: norm_history sets the clip; pass clip=None with it')
    matrix, was_host = engine.stage(users_grads)
    sq = engine.row_sqdist(matrix, np.zeros(matrix.shape[1], dtype=np.float32))
    norms = np.sqrt(sq.numpy() if isinstance(sq, DeviceBuffer) else sq.detach().cpu().numpy())
    norm_history.extend(float(v) for v in norms)
    history = np.asarray(norm_history, dtype=np.float64)
    history = history[np.isfinite(history)]
    threshold = min(float(np.median(history)), float(max_tau)) if history.size else 0.0
    if not threshold > 0.0:
        threshold = float(np.finfo(np.float64).tiny)        # (every norm 0 so far: nothing to clip to, every scale next to 0)
    got = engine.clipped_clustering(matrix, clip=threshold, method=method, distances=distances, sq=sq, return_info=return_info)
    if not was_host:
        return got
    return (got[0].numpy(), got[1]) if return_info else got.numpy()


def faba(users_grads, users_count, corrupted_count, distances=None, return_info=False):
    """FABA (Xia, Chen, Yu and Ma, IJCAI 2019; not in the reference): the mean of the clients is taken, the client farthest
    from it dropped, corrupted_count times over; the rest are averaged.  The oldest family of rules, iterative outlier
    removal, and the baseline the clustering defences here are compared with.  It runs on ONE pairwise distance matrix:
    the client farthest from the mean of a set is the client with the largest sum of squared distances to the set, and a
    removal takes one entry off every other client's sum, so the gradients are read for the distances and for the final
    mean and never in between.  A client with a NaN or infinite entry goes first and counts towards corrupted_count;
    identical clients tie and go lowest row first.  FABA removes what is FAR from the crowd: the drift attack's rows,
    which sit inside it, pass, as they pass `krum`.  `distances=` (a `Distances` handle or a dense matrix of Euclidean
    distances) replaces the distance stage.  Asserts users_count >= 2*corrupted_count + 1, as `multi_krum` does.  numpy
    in -> numpy out, device-resident in -> device-resident out.  return_info=True returns (vector, {kept_rows, order,
    removed, kept, forced, last_score, divisor}).  Not one of the `defend` keys: the reference's main.py offers only
    those four."""
    assert users_count >= 2 * corrupted_count + 1, ('users_count>=2*corrupted_count + 1', users_count, corrupted_count)
    return get_engine().faba(users_grads, users_count, corrupted_count, distances=distances, return_info=return_info)


class AfaReputation:
    """AFA's memory of who misbehaved (arXiv:1909.05125, section 3.2): client k's chance of sending a good update is
    Beta(alpha_k, beta_k), every client starting at (alpha0, beta0).  A round in which the rule kept the client adds 1 to its
    alpha, a round in which the rule removed it 1 to its beta, and its weight in the next round is the mean alpha / (alpha +
    beta).  A client is BLOCKED for good once P(p_k < 0.5) = I_0.5(alpha, beta) >= delta: its weight is 0 from then on, so the
    rule sees it as excluded.  Host-side, n small integers; for integer counts the regularised incomplete beta function is
    the exact binomial tail sum_{j = alpha}^{alpha + beta - 1} C(alpha + beta - 1, j) / 2^(alpha + beta - 1)."""

    def __init__(self, n, alpha0=3, beta0=3, delta=0.95):
        if int(alpha0) < 1 or int(beta0) < 1:
            raise ValueError('AfaReputation: alpha0 and beta0 are positive integers')
        self.alpha = np.full(int(n), int(alpha0), dtype=np.int64)
        self.beta = np.full(int(n), int(beta0), dtype=np.int64)
        self.blocked = np.zeros(int(n), dtype=bool)
        self.delta = float(delta)

    @staticmethod
    def bad_probability(alpha, beta):
        """I_0.5(alpha, beta) for positive integers: P(p < 0.5) under Beta(alpha, beta)."""
        import math
        alpha, beta = int(alpha), int(beta)
        trials = alpha + beta - 1
        return sum(math.comb(trials, j) for j in range(alpha, trials + 1)) / 2 ** trials

    def weights(self):
        """alpha / (alpha + beta) as float64, 0 for a blocked client.  A caller's sample counts multiply in on the host."""
        w = self.alpha / (self.alpha + self.beta)
        w[self.blocked] = 0.0
        return w

    def update(self, kept, excluded=()):
        """One round's outcome: `kept` and `excluded` are row indices.  A kept client's alpha grows by 1, a removed client's
        beta (removed: neither kept nor excluded); an excluded or blocked client is left alone.  Returns the clients blocked
        by this round."""
        n = self.alpha.size
        kept_mask, out_mask = np.zeros(n, dtype=bool), self.blocked.copy()
        kept_mask[np.asarray(kept, dtype=np.int64)] = True
        out_mask[np.asarray(excluded, dtype=np.int64)] = True
        self.alpha[kept_mask & ~out_mask] += 1
        removed = ~kept_mask & ~out_mask
        self.beta[removed] += 1
        fresh = [k for k in np.flatnonzero(removed) if self.bad_probability(self.alpha[k], self.beta[k]) >= self.delta]
        self.blocked[fresh] = True
        return np.asarray(fresh, dtype=np.int64)


def afa(users_grads, users_count, corrupted_count, weights=None, xi=2.0, delta_xi=0.5, gram=None, reputation=None):
    """AFA, Adaptive Federated Averaging (Munoz-Gonzalez, Co and Lupu, arXiv:1909.05125, Algorithm 1; not in the reference):
    every client's cosine with the weighted aggregate of the clients still kept is taken, the clients whose cosine lies more
    than xi standard deviations from the median are removed on the side the mean of the cosines points away from, xi grows by
    delta_xi, and the round repeats until it removes nobody; the rest are averaged with their weights.  It needs NO count of
    attackers: corrupted_count is accepted for the common signature and not used.  It runs on ONE fp64 Gram matrix (`gram=`
    replaces that stage) and reads the gradients for the Gram and for the final sum only.  The drift attack's copies of one
    vector have a cosine near 1 with the aggregate where an honest client's is small: the upper branch removes them, as the
    lower branch removes sign-flipped clients.  Clients of pure noise at three times the honest scale, and sign-flipped
    clients scaled by 3, are mostly KEPT: they drag the aggregate with them; put `weak_dp` or `centered_clip` in front for
    those.  A client with a NaN or zero gradient, or a weight that is not positive, is excluded.  `weights`: one fp64 weight a
    client (sample counts).  `reputation`: an `AfaReputation`; its weights multiply in, and it is updated with this round's
    kept and excluded clients.  numpy in -> numpy out, device-resident in -> device-resident out.  Usable as `then=` of
    `nnm`, `bucketing`, `robust_lr`, `sparsefed` and `weak_dp`.  Not one of the `defend` keys: the reference's main.py offers
    only those four."""
    engine = get_engine()
    if reputation is None:
        return engine.afa(users_grads, users_count, corrupted_count, weights=weights, xi=xi, delta_xi=delta_xi, gram=gram)
    w = reputation.weights()
    if weights is not None:
        w = w * np.asarray(weights.cpu() if hasattr(weights, 'cpu') else weights, dtype=np.float64).reshape(-1)
    out, info = engine.afa(users_grads, users_count, corrupted_count, weights=w, xi=xi, delta_xi=delta_xi, gram=gram,
                           return_info=True)
    reputation.update(info['kept_rows'], info['excluded_rows'])
    return out


class AurorHistory:
    """Auror's evidence carried over rounds (the paper gathers it over several): n int64 votes, n int32 bad flags and the 4
    int64 counts {indicative, clustered, capped, 0}, on the device, which every `auror(..., history=)` call adds to in place
    before it selects.  A client that once sent a non-finite value stays bad until `reset()`."""

    def __init__(self, n):
        engine = get_engine()
        self.n = int(n)
        self.votes = engine.empty((self.n,), np.int64)
        self.bad = engine.empty((self.n,), np.int32)
        self.counts = engine.empty((4,), np.int64)
        self.rounds = 0
        self.reset()

    def reset(self):
        """Forget every round: zero votes, flags and counts."""
        self.votes.upload(np.zeros(self.n, dtype=np.int64))
        self.bad.upload(np.zeros(self.n, dtype=np.int32))
        self.counts.upload(np.zeros(4, dtype=np.int64))
        self.rounds = 0

    def numpy(self):
        """(votes, bad, counts) as host arrays."""
        return self.votes.numpy(), self.bad.numpy(), self.counts.numpy()


def auror(users_grads, users_count, corrupted_count, alpha, tau=0.5, max_iter=32, history=None, return_info=False):
    """Auror (Shen, Tople and Saxena, ACSAC 2016; not in the reference): every coordinate's values over the clients are split
    into two clusters (2-means from the smallest and largest value), a coordinate whose two centres end more than `alpha`
    apart is indicative, and a client that sits in the smaller cluster of more than `tau` of the indicative coordinates is
    dropped; the rest are averaged.  The classic defence against TARGETED poisoning: a label flip or a backdoor moves a few
    coordinates a lot and leaves the rest alone.  The rule is column-local and reads the matrix once (up to 4096 clients).
    What it does not do: it is no answer to the drift attack, and `alpha` has NO default, because a unimodal coordinate of
    spread sigma splits into centres about 1.6 sigma apart -- with alpha below that every coordinate is indicative and
    honest clients are dropped (an "A Little Is Enough" matrix with alpha = 1.0 sigma lost 759 of 760 honest rows).  Choose
    it from `Engine.auror_votes(..., return_gap=True)`.  It needs NO count of attackers: corrupted_count is accepted for the
    common signature and not used.  A client with a NaN or infinite value is dropped.  `history`: an `AurorHistory`; this
    round's votes are added to it and the selection reads the sums (device-resident matrices; a host matrix is uploaded).
    numpy in -> numpy out, device-resident in -> device-resident out.  return_info=True returns (vector, {kept_rows, votes,
    bad, counts, gap, indicative, removed, kept, bad_rows, capped_cols}).  Usable as `then=` of `nnm`, `bucketing`,
    `robust_lr`, `sparsefed` and `weak_dp` (pass alpha= beside it).  Not one of the `defend` keys: the reference's main.py
    offers only those four."""
    engine = get_engine()
    if history is None:
        return engine.auror(users_grads, users_count, corrupted_count, alpha=alpha, tau=tau, max_iter=max_iter, return_info=return_info)
    matrix, was_host = engine.stage(users_grads)
    if matrix.shape[0] != history.n:
        raise ValueError('auror: the history holds %d clients, the gradients %d' % (history.n, matrix.shape[0]))
    got = engine.auror(matrix, users_count, corrupted_count, alpha=alpha, tau=tau, max_iter=max_iter, votes=history.votes,
                       bad=history.bad, counts=history.counts, return_info=return_info)
    history.rounds += 1
    if not was_host:
        return got
    return (got[0].numpy(), got[1]) if return_info else got.numpy()


class FoolsGoldHistory:
    """FoolsGold's memory of direction: the n x width float32 matrix of every client's updates summed over the rounds, on the
    device, zero at the start, which every `foolsgold(..., history=)` call adds this round's column window to in place before
    it takes the Gram.  Row i is client i, by position: every client reports every round.  A client that once sent a
    non-finite value has a non-finite row, and is excluded, until `reset()`.  `columns` is the (start, stop) window of the
    gradients the history is taken over (None until the first call fixes it); `rounds` counts the calls."""

    def __init__(self, n, width):
        engine = get_engine()
        self.n, self.width = int(n), int(width)
        if self.n < 1 or self.width < 1:
            raise ValueError('FoolsGoldHistory: n and width are positive')
        self.matrix = engine.empty((self.n, self.width), np.float32)
        self.columns = None
        self.rounds = 0
        self.reset()

    def reset(self):
        """Forget every round: a zero matrix."""
        self.matrix.upload(np.zeros((self.n, self.width), dtype=np.float32))
        self.rounds = 0

    def numpy(self):
        """The history as a host array."""
        return self.matrix.numpy()


def foolsgold(users_grads, users_count, corrupted_count, history=None, columns=None, kappa=1.0, normalise='count', gram=None,
              return_info=False):
    """FoolsGold (Fung, Yoon and Beschastnikh, arXiv:1808.04866; not in the reference): the defence against SYBILS, several
    clients that push one shared poisoning objective round after round.  Every client's largest cosine similarity with
    another client is taken over the ACCUMULATED updates (`history`: a `FoolsGoldHistory`, added to in place; None: this
    round's gradients alone), pardoned where the other client's own maximum is larger, and turned into a weight in [0, 1]
    by the clipped logit with confidence `kappa`; the result is the weighted sum of this round's gradients over the number
    of usable clients (normalise='count': with every weight 1 the rule is the mean) or over the weights' sum
    (normalise='sum').  It runs on ONE fp64 Gram matrix (`gram=` replaces that stage).  `columns`: None for all, or
    (start, stop): the window the similarity is taken over -- the paper uses the output layer on deep nets, and a
    full-width history of a large model does not fit beside its gradients.  It needs NO count of attackers: users_count
    and corrupted_count are accepted for the common signature and not used.  What it does NOT do: ONE attacker is
    invisible to it (it has nobody to resemble); honest clients with IID data point the same way and are penalised as
    if they were sybils; and it is no answer to the drift attack, whose rows sit inside the honest crowd round by round.
    A client whose history holds a NaN or an infinity is excluded.  Not built: the paper's feature-importance weighting
    and partial participation (clients are rows by position).  numpy in -> numpy out, device-resident in ->
    device-resident out.  return_info=True returns (vector, {weights, usable, excluded, at_zero, at_one, degenerate, top,
    divisor}).  Usable as `then=` of `nnm`, `bucketing`, `robust_lr`, `sparsefed` and `weak_dp`.  Not one of the `defend`
    keys: the reference's main.py offers only those four."""
    engine = get_engine()
    if history is None:
        return engine.foolsgold(users_grads, users_count, corrupted_count, columns=columns, kappa=kappa, normalise=normalise,
                                gram=gram, return_info=return_info)
    matrix, was_host = engine.stage(users_grads)
    n, d = (int(v) for v in matrix.shape)
    start, width = engine._foolsgold_window(d, columns)
    if (n, width) != (history.n, history.width):
        raise ValueError('foolsgold: the history holds %d clients x %d columns, the window is %d x %d'
                         % (history.n, history.width, n, width))
    if history.columns not in (None, (start, start + width)):
        raise ValueError('foolsgold: the history was gathered over the columns %r, not %r' % (history.columns, (start, start + width)))
    got = engine.foolsgold(matrix, users_count, corrupted_count, history=history.matrix, columns=(start, start + width), kappa=kappa,
                           normalise=normalise, gram=gram, return_info=return_info)
    history.columns = (start, start + width)
    history.rounds += 1
    if not was_host:
        return got
    return (got[0].numpy(), got[1]) if return_info else got.numpy()


def coordinate_median(users_grads, users_count, corrupted_count):
    """The coordinate-wise median (Yin et al. 2018; not in the reference): np.median of every column, bit for bit.  The
    reference's signature; users_count and corrupted_count are accepted and unused.  Not one of the `defend` keys: the
    reference's main.py offers only those four."""
    return get_engine().coordinate_median(users_grads)


def rank_trimmed_mean(users_grads, users_count, corrupted_count):
    """The beta-trimmed mean of Yin et al. 2018 (not in the reference): per column the corrupted_count smallest and the
    corrupted_count largest values dropped, the rest averaged (in fp64, rounded once).  A different rule from
    `trimmed_mean`, which keeps the values closest to the median.  Not one of the `defend` keys."""
    assert users_grads.shape[0] >= 2 * corrupted_count + 1, (
        'rows>=2*corrupted_count + 1', users_grads.shape[0], corrupted_count)
    return get_engine().rank_trimmed_mean(users_grads, corrupted_count)


def phocas(users_grads, users_count, corrupted_count):
    """Phocas (Xie, Koyejo and Gupta 2018; not in the reference): per column the corrupted_count-trimmed mean of Yin et al.
    (`rank_trimmed_mean`'s bits), then the mean of the rows - corrupted_count values nearest to it (in fp64, rounded once;
    ties in the distance go to the earlier row).  One library call, nothing read by the host.  The reference's signature;
    users_count is accepted and unused (the rows are counted).  numpy in -> numpy out, device-resident in -> device-resident
    out.  Not one of the `defend` keys: the reference's main.py offers only those four."""
    assert users_grads.shape[0] >= 2 * corrupted_count + 1, (
        'rows>=2*corrupted_count + 1', users_grads.shape[0], corrupted_count)
    return get_engine().phocas(users_grads, corrupted_count)


def mean_around(users_grads, users_count, corrupted_count, centre='median', keep=None):
    """Per column the mean of the `keep` values nearest to a centre (default keep: rows - corrupted_count), in fp64 and
    rounded once, ties in the distance going to the earlier row (Engine.window_mean).  centre='median': the coordinate-wise
    median, `coordinate_median`'s bits -- with the default keep this is "MeaMed", the mean around the median of Xie, Koyejo
    and Gupta 2018; the reference's `trimmed_mean` is the same rule with keep fixed at rows - corrupted_count - 1 and an
    fp32 finish.  centre='trimmed': the corrupted_count-trimmed mean, which with the default keep is `phocas`.  Or a vector
    of one float32 per column, on the device or the host.  A host matrix is uploaded once.  users_count is accepted and
    unused.  Not one of the `defend` keys."""
    rows = users_grads.shape[0]
    if keep is None:
        keep = rows - int(corrupted_count)
    if isinstance(centre, str) and centre not in ('median', 'trimmed'):
        raise ValueError("mean_around: centre is 'median', 'trimmed' or a vector, got %r" % (centre,))
    if not 1 <= int(keep) <= rows:
        raise ValueError('mean_around: keep %d outside 1..%d (the row count)' % (int(keep), rows))
    engine = get_engine()
    if not isinstance(centre, str):
        return engine.window_mean(users_grads, centre, keep)
    matrix, back = _upload_once(users_grads)
    if centre == 'median':
        around = engine.coordinate_median(matrix)
    else:
        assert rows >= 2 * corrupted_count + 1, ('rows>=2*corrupted_count + 1', rows, corrupted_count)
        around = engine.rank_trimmed_mean(matrix, corrupted_count)
    return back(engine.window_mean(matrix, around, keep))


def dnc(users_grads, users_count, corrupted_count, niters=1, filter_frac=1.0, sub_dim=10000, power_iters=32, seed=0,
        columns=None, return_index=False):
    """DnC, the spectral defence (Shejwalkar and Houmansadr, NDSS 2021, Algorithm 2; not in the reference): in each of
    `niters` iterations the rows are scored on `sub_dim` sampled columns by their squared projection on the top singular
    vector of the centred sample, the min(n - 1, int(filter_frac * corrupted_count)) highest scores removed; the rows every
    iteration kept are averaged (np.mean(users_grads[good], axis=0)).  The samples come from `dnc_columns(D, sub_dim,
    niters, seed)` unless `columns` gives them (one ascending list per iteration, which then sets niters and sub_dim).
    `return_index=True` returns the kept rows, ascending, instead.  users_count is accepted and unused (the rows are
    counted).  Not one of the `defend` keys: the reference's main.py offers only those four."""
    n, d = users_grads.shape
    remove_count = min(n - 1, int(filter_frac * corrupted_count))
    if columns is None:
        columns = dnc_columns(d, sub_dim, niters, seed)
    engine = get_engine()
    if return_index:
        return engine.dnc_select(users_grads, remove_count, columns, power_iters=power_iters)
    return engine.dnc(users_grads, remove_count, columns, power_iters=power_iters)


defend = {DefenseTypes.Krum: krum,
          DefenseTypes.TrimmedMean: trimmed_mean, DefenseTypes.NoDefense: no_defense,
          DefenseTypes.Bulyan: bulyan}
