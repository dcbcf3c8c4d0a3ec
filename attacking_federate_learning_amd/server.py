"""The server's round state on the GPU (reference server.py:33-36, 54-56, 81-90) -- SURVEY.md 8(a) rows a9/a10.

The reference's `Server` keeps `current_weights`, `velocity` and the N x D matrix `users_grads` as host numpy
arrays; every round the clients' gradients are copied into the matrix row by row (collect_gradients), the chosen
defence reduces it to one vector (defend) and a momentum step moves the weights.  `DeviceServer` keeps those three
arrays on the MI355X and runs the same three steps there, so a round never crosses PCIe:

    collect_gradients(users)        server.py:81-83   rows written by libbyzagg (host vectors or device tensors)
    collect_batched(net, x, y)      server.py:54-56 + user.py:76-92 for every client at once (clients.py)
    attack(attacker_rows, num_std)  main.py:68 -> malicious.py:10-36 on the first rows, in place
    attack_fang_trimmed_mean(rows)  Fang et al.'s attack on the trimmed mean / median on the same rows, fresh draws every round
    attack_fang_krum(rows)          Fang et al.'s attack on Krum on the same rows
    attack_minmax(rows)             Shejwalkar and Houmansadr's Min-Max / Min-Sum attack on the same rows
    defend(defence_method)          server.py:86-90  defences.defend[...] on the device matrix + fused momentum step
    defend_centered_clip(tau, iters)  the same step with centered clipping from the previous round's aggregate
    defend_fltrust(root_grad)         the same step with FLTrust against the server's own root gradient
    defend_signguard(frac, ...)       the same step with SignGuard, a new census window every round
    defend_nnm(then)                  the same step with nearest-neighbour mixing in front of the rule `then`
    defend_robust_lr(theta, then)     the same step with the robust learning rate round the mean or the rule `then`
    defend_bucketing(then, s)         the same step with s-bucketing, reshuffled every round, in front of the rule `then`
    defend_sparsefed(k, clip, then)   the same step with SparseFed: only the k heaviest coordinates of an error-feedback memory
    defend_weak_dp(clip, sigma, then) the same step with norm clipping and Gaussian noise drawn on the GPU, fresh every round
    defend_flame(lam, min_samples)    the same step with FLAME: the majority cluster by cosine distance, clipped, averaged, noised
    defend_clipped_clustering(method) the same step with ClippedClustering: the larger of two average-linkage clusters, clipped
    defend_faba()                     the same step with FABA: the clients farthest from the running mean dropped one by one
    defend_afa(xi, delta_xi)          the same step with AFA: cosine outliers dropped round after round, reputations kept across rounds
    defend_auror(alpha, tau)          the same step with Auror: per-coordinate 2-means, suspicion votes kept across rounds
    defend_foolsgold(columns, kappa)  the same step with FoolsGold: sybils' weights cut, the clients' summed updates kept across rounds
    defend_multi_metrics(p)           the same step with Multi-Metrics: the int(p n) clients of smallest Mahalanobis score, averaged

Only what is on the aggregation path is mirrored: evaluation, checkpoints, logging and data loading stay the
reference's own code.
"""
import numpy as np

from . import defences
from .assembly import GradientMatrix
from .engine import get_engine


class DeviceServer:
    def __init__(self, n_users, current_weights, mal_prop, learning_rate, momentum, torch_device='cuda', engine=None):
        import torch
        self.engine = engine or get_engine()
        self.n_users = int(n_users)
        self.mal_prop, self.learning_rate, self.momentum = mal_prop, learning_rate, momentum
        # server.py:33-36: weights as one flat fp32 row, the gradient matrix, a zero velocity
        self.current_weights = torch.as_tensor(np.asarray(current_weights, dtype=np.float32)).to(torch_device).clone()
        self.users_grads = GradientMatrix(self.n_users, self.current_weights.numel(), engine=self.engine,
                                          torch_device=torch_device)
        self.velocity = torch.zeros_like(self.current_weights)
        # centered clipping's history: the previous round's aggregate (zeros before the first round)
        self.clip_centre = torch.zeros_like(self.current_weights)
        # bucketing's history: the calls of defend_bucketing so far (the default seed of the next shuffle)
        self.bucketing_round = 0
        # SignGuard's history: the calls of defend_signguard so far (the default seed of the next window and sample)
        self.signguard_round = 0
        # SparseFed's history: the error-feedback memory W (zeros before the first round)
        self.sparse_residual = torch.zeros_like(self.current_weights)
        # weak DP's history: the calls of defend_weak_dp so far (the `round` of the next noise vector)
        self.weak_dp_round = 0
        # FLAME's history: the calls of defend_flame so far (the `round` of the next noise vector)
        self.flame_round = 0
        # the Fang trimmed-mean attack's history: the calls of attack_fang_trimmed_mean so far (the `round` of the next draws)
        self.fang_round = 0
        # ClippedClustering's history: the norms of every client of every round so far (the clip is their median)
        self.clipped_clustering_norms = []
        # AFA's history: the clients' reputations (made by the first defend_afa that asks for them)
        self.afa_reputation = None
        # Auror's history: the clients' votes and the indicative count summed over the rounds (made by the first defend_auror
        # that asks for it)
        self.auror_history = None
        # FoolsGold's history: every client's updates summed over the rounds (made by the first defend_foolsgold that asks for it)
        self.foolsgold_history = None

    # ---- server.py:81-83 ---------------------------------------------------------------------------
    def collect_gradients(self, users):
        self.users_grads.collect_gradients(users)

    # ---- server.py:54-56 + 81-83 with every client's step batched (user.py:76-92) --------------------
    def collect_batched(self, net, data, target):
        from .clients import collect_batched
        collect_batched(self.users_grads, net, self.current_weights, data, target)

    # ---- main.py:68: the first rows are the malicious clients (main.py:28) ---------------------------
    def attack(self, n_malicious, num_std):
        """A Little Is Enough on rows 0 .. n_malicious-1, in place (malicious.py:10-36); returns mean, std."""
        if n_malicious <= 0:
            return None, None
        rows = self.users_grads.data[:n_malicious]
        _, mean, std = self.engine.drift_attack(rows, num_std, write_back=(num_std != 0))
        return mean, std

    # ---- the adaptive attacks of Fang et al. on the same rows -------------------------------------------
    def attack_fang_trimmed_mean(self, n_malicious, b=2.0, partial=False, seed=0):
        """Fang et al.'s trimmed-mean / median attack on rows 0 .. n_malicious-1, in place (engine.fang_trmean_attack): every
        malicious row its own draws beyond the benign extremes (partial=True: from the malicious rows' own mean and std).
        `fang_round`, the calls so far, is passed as the stream's `round` and then incremented, as defend_weak_dp counts its
        own: one seed draws fresh numbers every round.  Nothing leaves the GPU; nothing synchronises."""
        if n_malicious <= 0:
            return None
        rows = self.engine.fang_trmean_attack(self.users_grads.data, n_malicious, b=b, partial=partial, seed=seed,
                                              round=self.fang_round)
        self.fang_round += 1
        return rows

    def attack_fang_krum(self, n_malicious, threshold=1e-5):
        """Fang et al.'s Krum attack on rows 0 .. n_malicious-1, in place (engine.fang_krum_attack): all of them become
        -lambda s.  Returns {lambda0, lambda, steps, chosen, succeeded}.  The gradients stay on the GPU; the host reads one
        index per halving of lambda."""
        if n_malicious <= 0:
            return None
        _, info = self.engine.fang_krum_attack(self.users_grads.data, n_malicious, threshold=threshold, return_info=True)
        return info

    def attack_minmax(self, n_malicious, kind='minmax', perturbation='std', partial=False):
        """The Min-Max / Min-Sum attack of Shejwalkar and Houmansadr on rows 0 .. n_malicious-1, in place
        (engine.minmax_attack): all of them become mu + gamma p.  Returns {gamma, bound, c, binding_row, known_rows, degenerate,
        broken}; reading it is the call's one synchronisation (Min-Max also waits where the distances wait).  The gradients
        stay on the GPU."""
        if n_malicious <= 0:
            return None
        _, info = self.engine.minmax_attack(self.users_grads.data, n_malicious, kind=kind, perturbation=perturbation,
                                            partial=partial, return_info=True)
        return info

    # ---- server.py:86-90 ---------------------------------------------------------------------------
    def defend(self, defence_method, cur_epoch=None):
        # one of the reference's four keys, or a rule of the reference's signature itself (defences.phocas, coordinate_median, ...)
        rule = defence_method if callable(defence_method) else defences.defend[defence_method]
        current_grads = rule(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop))
        # velocity = momentum * velocity - learning_rate * current_grads ; current_weights += velocity
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with centered clipping, the one defence that reads the round state -----------
    def defend_centered_clip(self, tau=10.0, iters=3):
        """Centered clipping of this round's gradients from `clip_centre`, the previous round's aggregate; the result is
        the next round's centre.  Then server.py:89-90's momentum step, as `defend` takes it."""
        current_grads = self.engine.centered_clip(self.users_grads.data, tau=tau, iters=iters, start=self.clip_centre)
        self.clip_centre.copy_(current_grads)     # a copy: the caller owns the aggregate it gets back
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with FLTrust, the one defence that takes the server's own gradient ------------
    def defend_fltrust(self, root_grad):
        """FLTrust of this round's gradients against `root_grad`, the gradient of the current weights on the server's own
        root dataset; then server.py:89-90's momentum step, as `defend` takes it.  Computing the root gradient is the
        caller's job; with clients.py it is one client's step on the root batch (root_x, root_y):

            root_grad = torch.cat([t.reshape(-1) for t in
                                   clients.per_client_gradients(net, server.current_weights, root_x[None], root_y[None])])
        """
        current_grads = self.engine.fltrust(self.users_grads.data, root_grad)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with SignGuard, whose window moves every round -----------------------------------
    def defend_signguard(self, frac=0.1, lower=0.1, upper=3.0, bandwidth=None, n_samples=50, seed=None):
        """SignGuard of this round's gradients (defences.signguard), then server.py:89-90's momentum step, as `defend` takes
        it.  seed=None takes `signguard_round`, the number of earlier calls of this method on this server, so that every
        round draws a new census window and a new sample, as the paper does."""
        if seed is None:
            seed = self.signguard_round
        self.signguard_round += 1
        current_grads = defences.signguard(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), frac=frac,
                                           lower=lower, upper=upper, bandwidth=bandwidth, n_samples=n_samples, seed=seed)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with nearest-neighbour mixing in front of a rule -------------------------------
    def defend_nnm(self, then, **then_kwargs):
        """Nearest-neighbour mixing of this round's gradients (every row the mean of its n - f nearest rows), the rule
        `then(mixed, n_users, n_malicious, **then_kwargs)` on the mixed matrix -- defences.krum, trimmed_mean,
        coordinate_median, geometric_median, ... --, then server.py:89-90's momentum step, as `defend` takes it.  The mixed
        matrix never leaves the device."""
        if not callable(then):
            raise TypeError('defend_nnm needs the rule to apply to the mixed matrix, e.g. defences.trimmed_mean')
        current_grads = defences.nnm(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), then=then,
                                     **then_kwargs)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with the robust learning rate round an aggregate ---------------------------------
    def defend_robust_lr(self, theta=None, then=None, **then_kwargs):
        """The robust learning rate on this round's gradients: the mean (then=None; vote and mean in one read of the matrix)
        or the rule `then(grads, n_users, n_malicious, **then_kwargs)` -- defences.trimmed_mean, coordinate_median, ... --
        with its sign inverted in every coordinate where the clients' sign vote stays below theta (default n_malicious + 1);
        then server.py:89-90's momentum step, as `defend` takes it.  With velocity = momentum*velocity - lr*grads a negated
        coordinate of grads is the paper's negated learning rate for that coordinate."""
        if then is not None and not callable(then):
            raise TypeError('defend_robust_lr: `then` is the rule to wrap, e.g. defences.trimmed_mean, or None for the mean')
        current_grads = defences.robust_lr(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), theta=theta,
                                           then=then, **then_kwargs)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with s-bucketing in front of a rule ----------------------------------------------
    def defend_bucketing(self, then, s=2, seed=None, **then_kwargs):
        """s-bucketing of this round's gradients (the clients shuffled, every s consecutive ones replaced by their mean), the
        rule `then(bucketed, ceil(n_users / s), n_malicious, **then_kwargs)` on the bucket means -- defences.krum,
        coordinate_median, geometric_median, centered_clip, ... --, then server.py:89-90's momentum step, as `defend` takes
        it.  The shuffle is bucketing_permutation(n_users, seed); seed=None takes `bucketing_round`, the number of earlier
        calls of this method on this server, so that every round reshuffles, as the paper requires.  The bucketed matrix never
        leaves the device."""
        if not callable(then):
            raise TypeError('defend_bucketing needs the rule to apply to the bucket means, e.g. defences.coordinate_median')
        if seed is None:
            seed = self.bucketing_round
        self.bucketing_round += 1
        current_grads = defences.bucketing(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), s=s,
                                           then=then, seed=seed, **then_kwargs)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with SparseFed, the one defence that keeps what it did not apply -------------------
    def defend_sparsefed(self, k=None, clip=10.0, then=None, **then_kwargs):
        """SparseFed on this round's gradients (defences.sparsefed): the clipped mean (then=None) or the rule `then(grads,
        n_users, n_malicious, **then_kwargs)` is added to `sparse_residual`, the error-feedback memory this server keeps
        (zeros at construction), the k coordinates of the memory with the largest magnitude (default max(1, D // 100)) are
        taken out of it as the step, and server.py:89-90's momentum step runs on that sparse vector, as `defend` takes it.
        With momentum = 0 this is the paper's Algorithm 1: a constant learning rate in front of W does not change which
        coordinates are largest, so scaling the step after the selection equals scaling the aggregates before it.  The
        paper's optional momentum sits BEFORE the memory (it smooths the aggregate that enters W); this server's sits AFTER
        it, on the sparse step, because the velocity is the reference's and every defend_* shares it."""
        if then is not None and not callable(then):
            raise TypeError('defend_sparsefed: `then` is the rule that supplies the aggregate, or None for the clipped mean')
        current_grads = defences.sparsefed(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), k=k, clip=clip,
                                           residual=self.sparse_residual, then=then, **then_kwargs)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with norm clipping and Gaussian noise ("weak DP") ----------------------------------------
    def defend_weak_dp(self, clip=10.0, sigma=0.01, adaptive=False, seed=0, then=None, **then_kwargs):
        """Clip and noise on this round's gradients (defences.weak_dp): every client clipped to norm `clip` (adaptive=True:
        to the median norm, the noise scaled by it) and averaged, or the rule `then(grads, n_users, n_malicious,
        **then_kwargs)`, then Gaussian noise of standard deviation sigma drawn on the GPU, and server.py:89-90's momentum
        step on the noisy vector, as `defend` takes it.  `weak_dp_round`, the calls so far, is passed as the stream's
        `round` and then incremented: one seed draws fresh noise every round, and a replayed round its own noise again."""
        if then is not None and not callable(then):
            raise TypeError('defend_weak_dp: `then` is the rule that supplies the aggregate, or None for the clipped mean')
        current_grads = defences.weak_dp(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), clip=clip,
                                         sigma=sigma, adaptive=adaptive, seed=seed, round=self.weak_dp_round, then=then,
                                         **then_kwargs)
        self.weak_dp_round += 1
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with FLAME ----------------------------------------------------------------------------------
    def defend_flame(self, lam=0.001, min_samples=1, seed=0):
        """FLAME on this round's gradients (defences.flame): the majority cluster by cosine distance, clipped to the median
        norm and averaged, Gaussian noise of standard deviation lam * (that median) drawn on the GPU, and server.py:89-90's
        momentum step on the result, as `defend` takes it.  `flame_round`, the calls so far, is passed as the stream's
        `round` and then incremented, as defend_weak_dp counts its own."""
        current_grads = defences.flame(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), lam=lam,
                                       min_samples=min_samples, seed=seed, round=self.flame_round)
        self.flame_round += 1
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with Multi-Metrics ---------------------------------------------------------------------------
    def defend_multi_metrics(self, p=0.3):
        """Multi-Metrics on this round's gradients (defences.multi_metrics): the int(p * n) clients of smallest Mahalanobis
        score over their summed Manhattan, Euclidean and cosine distances, averaged, and server.py:89-90's momentum step on
        the result, as `defend` takes it.  Stateless: nothing is carried from round to round."""
        current_grads = defences.multi_metrics(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), p=p)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with FABA -----------------------------------------------------------------------------------
    def defend_faba(self):
        """FABA on this round's gradients (defences.faba): int(n_users * mal_prop) times the client farthest from the mean of
        those still kept is dropped, the rest averaged, and server.py:89-90's momentum step on the result, as `defend` takes
        it.  Stateless: nothing is carried from round to round."""
        current_grads = defences.faba(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop))
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with AFA --------------------------------------------------------------------------------------
    def defend_afa(self, xi=2.0, delta_xi=0.5, reputation=True):
        """AFA on this round's gradients (defences.afa): the clients whose cosine with the aggregate lies too far from the
        median dropped, round after round, the rest averaged with their reputations as weights, and server.py:89-90's momentum
        step on the result, as `defend` takes it.  reputation=True keeps ONE `defences.AfaReputation` across the calls
        (`afa_reputation`): a client removed often enough is blocked for good.  reputation=False: stateless, unit weights."""
        if reputation and self.afa_reputation is None:
            self.afa_reputation = defences.AfaReputation(self.n_users)
        current_grads = defences.afa(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), xi=xi,
                                     delta_xi=delta_xi, reputation=self.afa_reputation if reputation else None)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with Auror ------------------------------------------------------------------------------------
    def defend_auror(self, alpha, tau=0.5, max_iter=32, history=True):
        """Auror on this round's gradients (defences.auror): every coordinate's values split in two, the clients in the smaller
        cluster of more than tau of the coordinates whose centres lie more than alpha apart dropped, the rest averaged, and
        server.py:89-90's momentum step on the result, as `defend` takes it.  alpha has no default (defences.auror says why).
        history=True keeps ONE `defences.AurorHistory` across the calls (`auror_history`), as the paper gathers its evidence
        over several rounds; history=False: stateless."""
        if history and self.auror_history is None:
            self.auror_history = defences.AurorHistory(self.n_users)
        current_grads = defences.auror(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop), alpha, tau=tau,
                                       max_iter=max_iter, history=self.auror_history if history else None)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with FoolsGold --------------------------------------------------------------------------------
    def defend_foolsgold(self, columns=None, kappa=1.0, normalise='count', history=True):
        """FoolsGold on this round's gradients (defences.foolsgold): the clients whose summed updates point the same way get
        their weight cut, the weighted sum is taken over the usable clients, and server.py:89-90's momentum step on the result,
        as `defend` takes it.  history=True keeps ONE `defences.FoolsGoldHistory` across the calls (`foolsgold_history`) over
        the window `columns` ((start, stop); None: every column) of the first such call; history=False: stateless, this
        round's cosines."""
        grads = self.users_grads.data
        if history and self.foolsgold_history is None:
            start, width = self.engine._foolsgold_window(grads.shape[1], columns)
            self.foolsgold_history = defences.FoolsGoldHistory(self.n_users, width)
        current_grads = defences.foolsgold(grads, self.n_users, int(self.n_users * self.mal_prop), columns=columns, kappa=kappa,
                                           normalise=normalise, history=self.foolsgold_history if history else None)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads

    # ---- the same step with ClippedClustering ----------------------------------------------------------------------
    def defend_clipped_clustering(self, method='average', max_tau=1e5):
        """ClippedClustering on this round's gradients (defences.clipped_clustering): the larger of the two average-linkage
        clusters by cosine distance, clipped to min(median of `clipped_clustering_norms`, max_tau) and averaged, and
        server.py:89-90's momentum step on the result, as `defend` takes it.  `clipped_clustering_norms` is the paper's
        running history: every call appends this round's norms to it (one read-back a round) before it takes the median."""
        current_grads = defences.clipped_clustering(self.users_grads.data, self.n_users, int(self.n_users * self.mal_prop),
                                                    method=method, norm_history=self.clipped_clustering_norms, max_tau=max_tau)
        self.engine.server_update(self.current_weights, self.velocity, current_grads, self.momentum,
                                  self.learning_rate)
        return current_grads
