"""Multi-GPU form of the hot path: one process per GPU, `torch.distributed` (backend "nccl" = RCCL over xGMI).

Two layouts of the N x D gradient matrix, both behind one `ShardedAggregator`:

  clients   rank r holds rows [r*N/W, (r+1)*N/W) of G with all D columns -- where the clients' gradients land
            (reference main.py:26-32, server.py:81-83; the layout BASELINE.json's north_star names).
            Distances: G is all-gathered one column PANEL at a time (RCCL all-gather of row tiles; the next panel's
            gather overlaps this panel's Gram); every rank then holds all N rows of the panel and computes ITS SHARE of
            the 128 x 128 Gram tiles (byz_gram_share_dev), the shares are summed by one fp64 all-reduce of N x N.
            Selection: replicated.  Bulyan's second stage needs every selected row per coordinate: the theta selected
            rows are re-sharded to column slices by one personalised exchange, the median-window mean runs per slice and
            the D-vector is all-gathered.
  columns   every rank holds all N rows of its own slice of the D columns.  trimmed_mean, no_defense and the attack are
            independent per column (no collective); the distance matrix is a sum over columns: each rank's fp64 Gram of
            its slice, ONE all-reduce of N x N doubles, replicated selection, local second stage.  Client-sharded input
            gets here through `reshard_clients_to_columns` (a personalised exchange of 1/W of the bytes an all-gather
            moves).

The all-reduce result is bitwise identical on every rank (each element is reduced in one fixed order and then broadcast),
so all ranks select the same clients; identical rows still tie exactly because the distance kernel canonicalises them.

`kernels` is the seam between this orchestration and the per-GPU kernels: the product uses `HipKernels` (libbyzagg on the
rank's GPU); the CPU test-suite drives the same orchestration over gloo with a numpy stand-in defined in tests/ -- there
is no CPU implementation in this package.  Every collective is timed and its bytes counted (`comm_report()`), because
which layout wins is a measurement, not an opinion.
"""
import time

import numpy as np


class HipKernels:
    """Per-rank kernels on the rank's own MI355X, operating on torch CUDA tensors."""

    def __init__(self, engine=None):
        from .engine import get_engine
        self.engine = engine or get_engine()

    def gram(self, g_local):
        return self.engine.gram(g_local)                       # (N, N) float64 CUDA tensor

    def gram_share(self, panel, row_index, share_count, share_index):
        return self.engine.gram_share(panel, row_index, share_count, share_index)

    def gram_accumulator(self, n, like):
        import torch
        return torch.zeros((n, n), dtype=torch.float64, device=like.device)

    def gram_share_add(self, panel, row_index, share_count, share_index, gram):
        return self.engine.gram_share_add(panel, row_index, share_count, share_index, gram)

    def pairwise_distances(self, g_local):
        return self.engine.pairwise_distances(g_local)         # Distances handle: Gram, distances, near pairs in one call

    def distances_from_gram(self, gram, local_columns=None, all_reduce=None):
        return self.engine.distances_from_gram(gram, gram.shape[0], local_columns=local_columns, all_reduce=all_reduce)

    def near_pairs_count(self):
        return self.engine.near_pairs_count()

    def near_pairs_sqdist(self, panel, count, row_index=None):
        return self.engine.near_pairs_sqdist(panel, count, row_index=row_index)

    def near_pairs_apply(self, sq, dist):
        self.engine.near_pairs_apply(sq, dist)

    def krum_select(self, dist, users_count, corrupted_count):
        return self.engine.krum_select(dist, users_count, corrupted_count)

    def bulyan_select(self, dist, users_count, corrupted_count, on_device=False):
        return self.engine.bulyan_select(dist, users_count, corrupted_count, on_device=on_device)

    def krum_bulyan_select(self, dist, users_count, corrupted_count, on_device=False):
        return self.engine.krum_bulyan_select(dist, users_count, corrupted_count, on_device=on_device)

    def multi_krum_select(self, dist, users_count, corrupted_count, m=None):
        return self.engine.multi_krum_select(dist, users_count, corrupted_count, m)

    def mean_rows(self, g_local, row_index):
        return self.engine.mean_rows(g_local, row_index)

    def nnm_neighbours(self, dist, k):
        return self.engine.nnm_neighbours(dist, k)            # (lists n x k, lengths n): int32, on the device

    def nnm_mix(self, g_local, neighbours, counts=None):
        return self.engine.nnm_mix(g_local, neighbours, counts)     # this rank's columns of the mixed matrix

    def bucket_means(self, g_local, s, perm):
        return self.engine.bucket_means(g_local, s, perm)     # this rank's columns of the bucket means

    def row_sqdist(self, g_local, z):
        return self.engine.row_sqdist(g_local, z)             # (N,) float64: this rank's part over its columns

    def weighted_mean(self, g_local, weights):
        # the weights come from this package (0/1 flags, 1 / max(nu, d)): no check, no host sync
        return self.engine.weighted_mean(g_local, weights, validate=False)

    def clip_update(self, g_local, v, scales):
        return self.engine.clip_update(g_local, v, scales)    # this rank's columns of the moved centre

    def row_dots(self, g_local, r):
        return self.engine.row_dots(g_local, r)               # two (N,) float64: this rank's parts over its columns

    def scaled_rows_sum(self, g_local, weights, divisor):
        return self.engine.scaled_rows_sum(g_local, weights, divisor)     # this rank's columns of the sum over the divisor

    def row_signs(self, g_local, window_start, window_len):
        # (pos, zero, neg, q): this rank's part of the counts over its part of the window, and of q over its columns
        return self.engine.row_signs(g_local, window_start, window_len)

    def signguard_select(self, pos, zero, neg, q, window_len, **kwargs):
        return self.engine.signguard_select(pos, zero, neg, q, window_len, **kwargs)     # the same on every rank

    def dnc_scores(self, g_local, columns, power_iters=32):
        return self.engine.dnc_scores(g_local, columns, power_iters=power_iters)     # one rank holds the sampled columns

    def dnc_select(self, g_local, remove_count, columns, power_iters=32):
        return self.engine.dnc_select(g_local, remove_count, columns, power_iters=power_iters)

    def dnc(self, g_local, remove_count, local_columns, sub_dim, power_iters=32, all_reduce=None, return_selection=False):
        # this rank's columns of the mean; the n-vectors of every iteration go through all_reduce (None: one rank)
        return self.engine.dnc_sharded(g_local, remove_count, local_columns, sub_dim, power_iters=power_iters,
                                       all_reduce=all_reduce, return_selection=return_selection)

    def trimmed_mean(self, g_local, corrupted_count, row_index=None):
        # row_index comes from this package (a selection the kernels produced): no bounds re-check, no host sync
        return self.engine.trimmed_mean(g_local, g_local.shape[0], corrupted_count, row_index=row_index,
                                        validate_index=False)

    def coordinate_median(self, g_local, row_index=None):
        return self.engine.coordinate_median(g_local, row_index=row_index, validate_index=False)

    def rank_trimmed_mean(self, g_local, trim_count, row_index=None):
        return self.engine.rank_trimmed_mean(g_local, trim_count, row_index=row_index, validate_index=False)

    def window_mean(self, g_local, centre_local, keep, row_index=None, return_radius=False):
        # column-local: this rank's slice of the matrix around this rank's slice of the centre
        return self.engine.window_mean(g_local, centre_local, keep, row_index=row_index, validate_index=False,
                                       return_radius=return_radius)

    def phocas(self, g_local, trim_count, row_index=None):
        return self.engine.phocas(g_local, trim_count, row_index=row_index, validate_index=False)

    def no_defense(self, g_local):
        return self.engine.no_defense(g_local)

    def sign_votes(self, g_local):
        return self.engine.sign_votes(g_local)                # this rank's columns of the votes: int32, on the device

    def robust_lr(self, g_local, theta, return_votes=False):
        return self.engine.robust_lr(g_local, theta, return_votes=return_votes)

    def topk_sparsify_sharded(self, x_local, k, n_total, rank, world, add=None, all_reduce=None, residual=None):
        # this rank's (step, memory) of the global top-k; the bins of every pass and the ranks' ties go through all_reduce
        return self.engine.topk_sparsify_sharded(x_local, k, n_total, rank, world, add=add, all_reduce=all_reduce,
                                                 residual=residual)

    def clip_scales(self, sq, clip=10.0, adaptive=False):
        # (scales, clip) from the all-reduced squared norms: the same on every rank; the clip stays on the device
        return self.engine.clip_scales(sq, clip=clip, adaptive=adaptive, return_clip=True)

    def gaussian_noise(self, x_local, sigma, seed=0, round=0, column_offset=0, scale=None):
        # this rank's columns of the noisy vector, in place: column_offset is the global index of its first column
        return self.engine.gaussian_noise(x_local, sigma, seed=seed, round=round, column_offset=column_offset, scale=scale,
                                          out=x_local)

    def cosine_from_gram(self, gram):
        return self.engine.cosine_from_gram(gram)             # Distances handle from the all-reduced Gram: the same on every rank

    def flame_select(self, dist, like, min_samples=1, min_cluster_size=None):
        # (0 / 1 flags of the admitted rows: an int32 tensor beside `like`; info): the same on every rank
        return self.engine.flame_select(dist, min_samples=min_samples, min_cluster_size=min_cluster_size, on_device=True, like=like)

    def clipped_clustering_select(self, dist, like, method='average', fill=2.0):
        # (0 / 1 flags of the admitted rows: an int32 tensor beside `like`; info): the same on every rank
        return self.engine.clipped_clustering_select(dist, method=method, fill=fill, on_device=True, like=like)

    def faba_select(self, dist, remove_count, like, power=2):
        # (0 / 1 flags of the kept rows: an int32 tensor beside `like`; info): the same on every rank
        return self.engine.faba_select(dist, remove_count, power=power, on_device=True, like=like)

    def afa_select(self, gram, like, weights=None, xi=2.0, delta_xi=0.5, max_rounds=None):
        # (0 / 1 flags of the kept rows: an int32 tensor beside `like`; info): the same on every rank
        return self.engine.afa_select(gram, weights=weights, xi=xi, delta_xi=delta_xi, max_rounds=max_rounds, on_device=True,
                                      like=like)

    def auror_votes(self, g_local, alpha, max_iter=32):
        # (votes int64, bad int32, counts int64[4]) of this rank's columns, on the device: additive over the column slices
        return self.engine.auror_votes(g_local, alpha, max_iter=max_iter)

    def auror_select(self, votes, bad, counts, like, tau=0.5):
        # (0 / 1 flags of the kept rows: an int32 tensor beside `like`; info): the same on every rank
        return self.engine.auror_select(votes, bad, counts, tau=tau, on_device=True, like=like)

    def rows_add(self, history, g_local, columns=None):
        return self.engine.rows_add(history, g_local, columns=columns)      # history += g_local[:, start:stop], in place

    def foolsgold_weights(self, gram, like, kappa=1.0, normalise='count'):
        # (n fp64 weights: a tensor beside `like`; info, whose divisor is T): the same on every rank
        return self.engine._foolsgold_weights(gram, kappa, normalise, True, like)

    def manhattan_sums(self, g_local):
        return self.engine.manhattan_sums(g_local)             # (N, N) float64 CUDA tensor: additive over the column slices

    def manhattan_from_sums(self, sums):
        return self.engine.manhattan_from_sums(sums)           # Distances handle from the all-reduced sums: the same on every rank

    def multi_metrics_select(self, man, euc, cos, keep, like):
        # (0 / 1 flags of the chosen rows: an int32 tensor beside `like`; info): the same on every rank
        features = self.engine.multi_metrics_features(man, euc, cos)
        return self.engine.multi_metrics_select(features, keep, on_device=True, like=like)

    def minmax_attack(self, g_local, n_malicious, kind, perturbation, partial, all_reduce=None, return_info=False):
        # in place on this rank's slice; the moments (and with 'unit' the mean's norm) go through all_reduce (None: one rank)
        return self.engine.minmax_attack(g_local, n_malicious, kind=kind, perturbation=perturbation, partial=partial,
                                         all_reduce=all_reduce, return_info=return_info)

    def drift(self, rows_local, num_std, write_back=False):
        return self.engine.drift_attack(rows_local, num_std, write_back=write_back)

    def column_chain(self, rows_local, carry=None, mean=None):
        return self.engine.column_chain(rows_local, carry=carry, mean=mean)

    def column_finish(self, total_rows, num_std, sum=None, sumsq=None, mean=None):
        return self.engine.column_finish(total_rows, num_std, sum=sum, sumsq=sumsq, mean=mean)

    def row(self, g_local, index):
        return g_local[index].clone()


class ShardedAggregator:
    """defences.py / malicious.py over a sharded gradient matrix (see the module docstring for the two layouts)."""

    def __init__(self, kernels, group=None):
        import os
        import torch.distributed as dist
        self.dist = dist
        self.kernels = kernels
        self.group = group
        self.world = dist.get_world_size(group) if dist.is_initialized() else 1
        self.rank = dist.get_rank(group) if dist.is_initialized() else 0
        # BYZ_FORCE_COLLECTIVES=1 issues the collectives even at world size 1 (exercises the RCCL path on one GPU)
        self.always_collective = dist.is_initialized() and os.environ.get('BYZ_FORCE_COLLECTIVES') == '1'
        self._comm = {}
        self._pending = []

    # ---- collectives, timed ------------------------------------------------------------------------------------
    def _collective(self):
        return self.world > 1 or self.always_collective

    def _timed(self, name, nbytes, tensor, fn, count=True):
        """Run one collective, book its bytes and its duration (device events for CUDA tensors)."""
        rec = self._comm.setdefault(name, {'calls': 0, 'bytes': 0, 'ms': 0.0})
        if count:
            rec['calls'] += 1
            rec['bytes'] += int(nbytes)
        if getattr(tensor, 'is_cuda', False):
            import torch
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = fn()
            stop.record()
            self._pending.append((name, start, stop))
            return out
        t0 = time.perf_counter()
        out = fn()
        rec['ms'] += (time.perf_counter() - t0) * 1e3
        return out

    def comm_report(self, reset=True):
        """{collective: {calls, bytes, ms}} since the last report; bytes are what THIS rank receives."""
        for name, start, stop in self._pending:
            stop.synchronize()
            self._comm[name]['ms'] += start.elapsed_time(stop)
        self._pending = []
        out = {k: dict(v) for k, v in self._comm.items()}
        if reset:
            self._comm = {}
        return out

    def _all_reduce(self, name, tensor):
        if self._collective():
            nbytes = tensor.numel() * tensor.element_size() * 2 * (self.world - 1) // max(self.world, 1)
            self._timed(name, nbytes, tensor,
                        lambda: self.dist.all_reduce(tensor, op=self.dist.ReduceOp.SUM, group=self.group))
        return tensor

    # ---- distances: the one bulk exchange of the path -----------------------------------------------------------
    def global_distances(self, g_local):
        """columns layout: Gram of the local slice, one all-reduce, distances (near-duplicate pairs re-evaluated on
        the difference: per-rank partial sums over the local columns, one more small all-reduce)."""
        if not self._collective() and hasattr(self.kernels, 'pairwise_distances'):
            # one rank holds every column: the engine's own composition, in which rows that its duplicate search has compared
            # byte for byte need no second proof through the near-pair exchange
            return self.kernels.pairwise_distances(g_local)
        gram = self.kernels.gram(g_local)
        self._all_reduce('allreduce_gram', gram)
        reduce_pairs = (lambda t: self._all_reduce('allreduce_near_pairs', t)) if self._collective() else None
        return self.kernels.distances_from_gram(gram, local_columns=g_local, all_reduce=reduce_pairs)

    def client_distances(self, rows_local, rows_per_rank, panel_columns=None):
        """clients layout: all-gather of column panels overlapped with this rank's share of the Gram tiles, then one
        all-reduce of the N x N fp64 Gram.  `rows_local`: this rank's (n_r, D) rows."""
        import torch
        n_max = int(max(rows_per_rank))
        n_mine, d = rows_local.shape
        assert n_mine == rows_per_rank[self.rank]
        if panel_columns is None:   # ~1 GiB of gathered panel, at least a few thousand columns
            panel_columns = max(4096, min(d, (1 << 28) // max(n_max * self.world, 1)))
        panel_columns = int(min(panel_columns, d))
        n_panels = -(-d // panel_columns)
        device = rows_local.device
        # logical row -> physical row of the gathered (W * n_max)-row panel (ranks with fewer rows are padded)
        row_index = np.concatenate([r * n_max + np.arange(rows_per_rank[r]) for r in range(self.world)]).astype(np.int32)
        even = all(c == n_max for c in rows_per_rank)
        row_index_t = None if even else torch.from_numpy(row_index).to(device)
        panels = [torch.empty((self.world * n_max, panel_columns), dtype=rows_local.dtype, device=device) for _ in range(2)]
        stage = [torch.zeros((n_max, panel_columns), dtype=rows_local.dtype, device=device) for _ in range(2)]

        class _Requests:
            """The requests of one panel's gather as one waitable."""
            def __init__(self, reqs):
                self.reqs = reqs

            def wait(self):
                for req in self.reqs:
                    req.wait()

        def start_gather(k):
            """All-gather of panel k's row tiles as point-to-point transfers over the xGMI full mesh: every rank sends its
            tile to each peer and receives each peer's tile straight into that peer's rows of the panel -- all seven links of
            a GPU busy at once, where the ring of `all_gather_into_tensor` is bound by ONE 153 GB/s link (VERDICT r3 weak 10;
            `_exchange` already moved the selected rows this way).  Same bytes, same result."""
            lo = k * panel_columns
            width = min(panel_columns, d - lo)
            src, dst = stage[k % 2], panels[k % 2]
            src[:n_mine, :width].copy_(rows_local[:, lo:lo + width])
            if not self._collective():
                dst[:n_max].copy_(src)
                return None, width
            rec = self._comm.setdefault('allgather_row_tiles', {'calls': 0, 'bytes': 0, 'ms': 0.0})
            rec['calls'] += 1
            rec['bytes'] += (self.world - 1) * n_max * width * src.element_size()
            ops = []
            for peer in range(self.world):
                mine_here = dst[peer * n_max:(peer + 1) * n_max]
                if peer == self.rank and not self.always_collective:
                    mine_here.copy_(src)
                    continue
                global_peer = self.dist.get_global_rank(self.group, peer) if self.group is not None else peer
                ops.append(self.dist.P2POp(self.dist.isend, src, global_peer, group=self.group))
                ops.append(self.dist.P2POp(self.dist.irecv, mine_here, global_peer, group=self.group))
            return _Requests(self.dist.batch_isend_irecv(ops)), width

        def sweep(per_panel):
            """Gather every panel once; panel k+1 is in flight while per_panel(k, panel) runs.  The booked time of the
            gathers is what the compute stream spent WAITING for them (the exposed part)."""
            pending = start_gather(0)
            for k in range(n_panels):
                work, width = pending
                if work is not None:
                    self._timed('allgather_row_tiles', 0, stage[0], work.wait, count=False)
                if k + 1 < n_panels:
                    pending = start_gather(k + 1)
                per_panel(k, panels[k % 2][:, :width])

        acc = {}
        # the panels' shares accumulate in ONE caller-owned N x N fp64 buffer inside the reduction kernel
        # (byz_gram_share_add_dev): no N x N `add_` pass per panel (128 MB per panel at N = 4000, ~150 panels at D = 1e7)
        gram = self.kernels.gram_accumulator(int(sum(rows_per_rank)), rows_local)

        def gram_of(k, panel):
            self.kernels.gram_share_add(panel, row_index_t, self.world, self.rank, gram)
        sweep(gram_of)
        self._all_reduce('allreduce_gram', gram)
        dist_m = self.kernels.distances_from_gram(gram)
        # pairs the Gram identity cannot resolve (near-duplicate clients) are re-evaluated on the difference itself
        # (defences.py:20): a second sweep, every rank takes the panels k = rank mod W, one small all-reduce
        count = self.kernels.near_pairs_count()
        if count:
            def pairs_of(k, panel):
                if k % self.world == self.rank:
                    part = self.kernels.near_pairs_sqdist(panel, count, row_index=row_index_t)
                    acc['sq'] = part if 'sq' not in acc else acc['sq'].add_(part)
            sweep(pairs_of)
            if 'sq' not in acc:
                acc['sq'] = torch.zeros(count, dtype=torch.float64, device=device)
            self._all_reduce('allreduce_near_pairs', acc['sq'])
            self.kernels.near_pairs_apply(acc['sq'], dist_m)
        return dist_m

    # ---- defences.py, columns layout --------------------------------------------------------------------------------
    def no_defense(self, g_local, users_count=None, corrupted_count=None, gather=False, total_columns=None):
        return self._maybe_gather(self.kernels.no_defense(g_local), gather, total_columns)

    def trimmed_mean(self, g_local, users_count, corrupted_count, gather=False, total_columns=None):
        return self._maybe_gather(self.kernels.trimmed_mean(g_local, corrupted_count), gather, total_columns)

    def coordinate_median(self, g_local, users_count=None, corrupted_count=None, gather=False, total_columns=None):
        """columns layout: np.median per column of the rank's own slice; no collective."""
        return self._maybe_gather(self.kernels.coordinate_median(g_local), gather, total_columns)

    def rank_trimmed_mean(self, g_local, users_count, corrupted_count, gather=False, total_columns=None):
        """columns layout: per column of the rank's own slice the corrupted_count smallest and largest values dropped, the
        rest averaged; no collective."""
        assert g_local.shape[0] >= 2 * corrupted_count + 1, (
            'rows>=2*corrupted_count + 1', g_local.shape[0], corrupted_count)
        return self._maybe_gather(self.kernels.rank_trimmed_mean(g_local, corrupted_count), gather, total_columns)

    def window_mean(self, g_local, centre_local, keep, gather=False, total_columns=None):
        """columns layout: per column of the rank's own slice the mean of the `keep` values nearest to the rank's slice of the
        centre (Engine.window_mean); no collective."""
        return self._maybe_gather(self.kernels.window_mean(g_local, centre_local, keep), gather, total_columns)

    def phocas(self, g_local, users_count, corrupted_count, gather=False, total_columns=None):
        """columns layout: Phocas per column of the rank's own slice -- the corrupted_count-trimmed mean, then the mean of the
        rows - corrupted_count values nearest to it; no collective."""
        assert g_local.shape[0] >= 2 * corrupted_count + 1, (
            'rows>=2*corrupted_count + 1', g_local.shape[0], corrupted_count)
        return self._maybe_gather(self.kernels.phocas(g_local, corrupted_count), gather, total_columns)

    def robust_lr(self, g_local, users_count, corrupted_count, theta=None, gather=False, total_columns=None):
        """The robust learning rate round the mean, columns layout: the sign vote and the mean are local to a column, so
        every rank makes the single-GPU call on its own slice (default theta: corrupted_count + 1); no collective."""
        if theta is None:
            theta = int(corrupted_count) + 1
        return self._maybe_gather(self.kernels.robust_lr(g_local, theta), gather, total_columns)

    def sparsefed(self, g_local, users_count, corrupted_count, k, clip=10.0, residual_local=None, total_columns=None,
                  gather=False):
        """SparseFed (defences.sparsefed's contract with then=None), columns layout: the clipped mean is this aggregator's
        centered_clip(iters=1) -- one all-reduce of N doubles --, and the top-k, the one step that is NOT local to a column,
        is kernels.topk_sparsify_sharded: four all-reduces (2048, 1024, 1024 and `world` doubles) whatever the data.  k and
        total_columns are the global figures (total_columns is needed beyond one rank); residual_local is this rank's slice
        of the memory, updated in place when given (None: zeros).  Returns (step, residual), this rank's columns of each
        (gather=True: the whole step)."""
        import torch
        n, d_local = g_local.shape
        if self.world > 1 and total_columns is None:
            raise ValueError('sparsefed() over several ranks needs total_columns')
        total = int(total_columns) if total_columns is not None else int(d_local)
        agg = self.centered_clip(g_local, tau=clip, iters=1)
        if residual_local is None:
            residual_local = torch.zeros(d_local, dtype=torch.float32, device=g_local.device)
        reduce = (lambda t: self._all_reduce('allreduce_topk', t)) if self._collective() else None
        out, res = self.kernels.topk_sparsify_sharded(residual_local, k, total, self.rank, self.world, add=agg, all_reduce=reduce,
                                                      residual=residual_local)
        return self._maybe_gather(out, gather, total_columns), res

    def weak_dp(self, g_local, users_count, corrupted_count, column_offset, clip=10.0, sigma=0.01, adaptive=False, seed=0,
                round=0, gather=False, total_columns=None, return_info=False):
        """Clip and noise (defences.weak_dp's contract with then=None), columns layout, both modes.  There is no sharded
        library call to make: a rank's squared norms cover its columns -- ONE all-reduce of N doubles makes them whole, the
        one centered_clip(iters=1) makes --, kernels.clip_scales then gives the same scales and clip on every rank, the
        clipped mean is local to the columns (kernels.clip_update from zero) and so is the noise, given column_offset, the
        global index of this rank's first column: the Philox stream is addressed by global column, so the ranks' slices
        concatenate to the single-GPU vector.  adaptive=True: the clip is the median norm and the noise sigma * clip, read
        on the device.  Returns this rank's columns (gather=True: the whole vector)."""
        import torch
        n, d_local = g_local.shape
        zero = torch.zeros(d_local, dtype=torch.float32, device=g_local.device)
        sq = self.kernels.row_sqdist(g_local, zero)
        self._all_reduce('allreduce_weak_dp_norms', sq)
        scales, used = self.kernels.clip_scales(sq, clip=clip, adaptive=adaptive)
        v = self.kernels.clip_update(g_local, zero, scales)
        if float(sigma) != 0.0:
            v = self.kernels.gaussian_noise(v, sigma, seed=seed, round=round, column_offset=column_offset,
                                            scale=used if adaptive else None)
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        d = torch.sqrt(sq)
        finite = torch.isfinite(d)
        return out, {'clipped_rows': int((finite & (d > used)).sum().item()), 'excluded_rows': int((~finite).sum().item()),
                     'clip': float(used.item())}

    def flame(self, g_local, users_count, corrupted_count, column_offset, lam=0.001, min_samples=1, min_cluster_size=None,
              seed=0, round=0, gather=False, total_columns=None, return_info=False):
        """FLAME (defences.flame's contract), columns layout.  TWO all-reduces: the N x N fp64 Gram of the ranks' slices and
        the N squared norms.  Everything after them is replicated -- kernels.cosine_from_gram, kernels.flame_select and
        kernels.clip_scales (adaptive) give the same flags, scales and clip on every rank -- or local to the columns: the
        sum of the admitted rows over their count, and the noise, given column_offset, the global index of this rank's first
        column (the Philox stream is addressed by global column).  Returns this rank's columns (gather=True: the whole
        vector)."""
        import torch
        n, d_local = g_local.shape
        gram = self.kernels.gram(g_local)
        self._all_reduce('allreduce_flame_gram', gram)
        dist = self.kernels.cosine_from_gram(gram)
        admitted, info = self.kernels.flame_select(dist, g_local, min_samples=min_samples, min_cluster_size=min_cluster_size)
        zero = torch.zeros(d_local, dtype=torch.float32, device=g_local.device)
        sq = self.kernels.row_sqdist(g_local, zero)
        self._all_reduce('allreduce_flame_norms', sq)
        scales, used = self.kernels.clip_scales(sq, adaptive=True)
        weights = torch.where(admitted != 0, scales, torch.zeros_like(scales))
        count = (admitted != 0).sum().to(torch.float64).reshape(1)
        v = self.kernels.scaled_rows_sum(g_local, weights, count)
        if float(lam) != 0.0:
            v = self.kernels.gaussian_noise(v, lam, seed=seed, round=round, column_offset=column_offset, scale=used)
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        info = dict(info, clip=float(used.item()), admitted_rows=torch.nonzero(admitted).reshape(-1).cpu().numpy())
        return out, info

    def clipped_clustering(self, g_local, users_count, corrupted_count, clip=None, method='average', fill=2.0, gather=False,
                           total_columns=None, return_info=False):
        """ClippedClustering (defences.clipped_clustering's contract), columns layout.  TWO all-reduces: the N x N fp64 Gram of
        the ranks' slices and the N squared norms.  Everything after them is replicated -- kernels.cosine_from_gram,
        kernels.clipped_clustering_select and kernels.clip_scales (clip=None: the median norm) give the same flags, scales
        and clip on every rank -- or local to the columns: the sum of the admitted rows over their count.  Returns this
        rank's columns (gather=True: the whole vector)."""
        import torch
        n, d_local = g_local.shape
        gram = self.kernels.gram(g_local)
        self._all_reduce('allreduce_clipped_clustering_gram', gram)
        dist = self.kernels.cosine_from_gram(gram)
        admitted, info = self.kernels.clipped_clustering_select(dist, g_local, method=method, fill=fill)
        zero = torch.zeros(d_local, dtype=torch.float32, device=g_local.device)
        sq = self.kernels.row_sqdist(g_local, zero)
        self._all_reduce('allreduce_clipped_clustering_norms', sq)
        scales, used = self.kernels.clip_scales(sq, clip=1.0 if clip is None else clip, adaptive=clip is None)
        weights = torch.where(admitted != 0, scales, torch.zeros_like(scales))
        count = (admitted != 0).sum().to(torch.float64).reshape(1)
        v = self.kernels.scaled_rows_sum(g_local, weights, count)
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        info = dict(info, clip=float(used.item()), admitted_rows=torch.nonzero(admitted).reshape(-1).cpu().numpy())
        return out, info

    def multi_metrics(self, g_local, users_count, corrupted_count, p=0.3, gather=False, total_columns=None, return_info=False):
        """Multi-Metrics (defences.multi_metrics' contract), columns layout.  The Gram's all-reduce (shared by the Euclidean
        and the cosine matrix) and ONE more of n x n doubles: the L1 sums, which are additive over the column slices.
        Everything after them is replicated -- kernels.manhattan_from_sums, kernels.cosine_from_gram and
        kernels.multi_metrics_select give the same flags on every rank -- or local to the columns: the mean of the chosen
        rows.  Returns this rank's columns (gather=True: the whole vector)."""
        import torch
        from .engine import Engine
        n = g_local.shape[0]
        keep = Engine._multi_metrics_keep(n, p=p)             # (a rank-local argument error: before any collective)
        gram = self.kernels.gram(g_local)
        self._all_reduce('allreduce_multi_metrics_gram', gram)
        reduce_pairs = (lambda t: self._all_reduce('allreduce_near_pairs', t)) if self._collective() else None
        euc = self.kernels.distances_from_gram(gram, local_columns=g_local, all_reduce=reduce_pairs)
        cos = self.kernels.cosine_from_gram(gram)
        sums = self.kernels.manhattan_sums(g_local)
        self._all_reduce('allreduce_multi_metrics_l1', sums)
        man = self.kernels.manhattan_from_sums(sums)
        flags, info = self.kernels.multi_metrics_select(man, euc, cos, keep, g_local)
        chosen = torch.nonzero(flags).reshape(-1).to(torch.int32)
        if chosen.numel() == 0:
            v = torch.zeros(g_local.shape[1], dtype=torch.float32, device=g_local.device)
        else:
            v = self.kernels.mean_rows(g_local, chosen)
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        return out, dict(info, chosen_rows=chosen.cpu().numpy().astype(np.int64))

    def krum(self, g_local, users_count, corrupted_count, return_index=False, gather=False, total_columns=None):
        if not return_index:
            assert users_count >= 2 * corrupted_count + 1, (
                'users_count>=2*corrupted_count + 3', users_count, corrupted_count)
        dist_m = self.global_distances(g_local)
        index = self.kernels.krum_select(dist_m, users_count, corrupted_count)
        if return_index:
            return index
        return self._maybe_gather(self.kernels.row(g_local, index), gather, total_columns)

    def bulyan(self, g_local, users_count, corrupted_count, gather=False, return_selection=False, total_columns=None):
        assert users_count >= 4 * corrupted_count + 3
        dist_m = self.global_distances(g_local)
        # the selection stays on the device between the loop and the second stage
        selection = self.kernels.bulyan_select(dist_m, users_count, corrupted_count, on_device=True)
        out = self.kernels.trimmed_mean(g_local, 2 * corrupted_count, row_index=selection)
        out = self._maybe_gather(out, gather, total_columns)
        if return_selection:
            host = selection.numpy() if hasattr(selection, 'numpy') else selection
            return out, np.asarray(host, dtype=np.int32)
        return out

    def multi_krum(self, g_local, users_count, corrupted_count, m=None, gather=False, return_selection=False,
                   total_columns=None):
        """Multi-Krum, columns layout: the distances' one all-reduce, the selection replicated on every rank, then every
        rank's mean of its own columns of the selected rows in ascending row order."""
        assert users_count >= 2 * corrupted_count + 1, (
            'users_count>=2*corrupted_count + 3', users_count, corrupted_count)
        dist_m = self.global_distances(g_local)
        selection = np.asarray(self.kernels.multi_krum_select(dist_m, users_count, corrupted_count, m), dtype=np.int32)
        out = self.kernels.mean_rows(g_local, np.sort(selection))
        out = self._maybe_gather(out, gather, total_columns)
        return (out, selection) if return_selection else out

    def faba(self, g_local, users_count, corrupted_count, gather=False, total_columns=None, return_info=False):
        """FABA (defences.faba's contract), columns layout.  No collective of its own: the distances' all-reduce of the N x N
        fp64 Gram (global_distances) is the only bulk exchange.  Everything after it is replicated -- kernels.faba_select
        gives the same flags on every rank -- or local to the columns: the sum of the kept rows over their count.  Returns
        this rank's columns (gather=True: the whole vector)."""
        import torch
        assert users_count >= 2 * corrupted_count + 1, ('users_count>=2*corrupted_count + 1', users_count, corrupted_count)
        dist_m = self.global_distances(g_local)
        kept, info = self.kernels.faba_select(dist_m, corrupted_count, g_local)
        weights = (kept != 0).to(torch.float64)
        v = self.kernels.scaled_rows_sum(g_local, weights, weights.sum().reshape(1))
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        return out, dict(info, kept_rows=torch.nonzero(kept).reshape(-1).cpu().numpy())

    def afa(self, g_local, users_count=None, corrupted_count=None, weights=None, xi=2.0, delta_xi=0.5, max_rounds=None,
            gather=False, total_columns=None, return_info=False):
        """AFA (defences.afa's contract), columns layout.  ONE all-reduce: the N x N fp64 Gram of the ranks' slices, the
        exchange the distances make.  Everything after it is replicated -- kernels.afa_select gives the same flags, weights and
        divisor on every rank -- or local to the columns: the weighted sum of the kept rows over their weights' sum.  Returns
        this rank's columns (gather=True: the whole vector)."""
        import torch
        n = g_local.shape[0]
        gram = self.kernels.gram(g_local)
        self._all_reduce('allreduce_gram', gram)
        kept, info = self.kernels.afa_select(gram, g_local, weights=weights, xi=xi, delta_xi=delta_xi, max_rounds=max_rounds)
        w = torch.ones(n, dtype=torch.float64, device=g_local.device) if weights is None else \
            torch.as_tensor(weights, dtype=torch.float64).to(g_local.device).reshape(-1)
        w = torch.where(kept != 0, w, torch.zeros_like(w))
        divisor = torch.tensor([info['divisor']], dtype=torch.float64, device=g_local.device)     # (the selection's own sum)
        v = self.kernels.scaled_rows_sum(g_local, w, divisor)
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        return out, dict(info, kept_rows=torch.nonzero(kept).reshape(-1).cpu().numpy())

    def auror(self, g_local, users_count=None, corrupted_count=None, alpha=None, tau=0.5, max_iter=32, gather=False,
              total_columns=None, return_info=False):
        """Auror (defences.auror's contract), columns layout.  The vote is column-local, so every rank makes the single-GPU
        call on its own slice; ONE all-reduce of the n votes, n bad flags and 4 counts as int64 (2 n + 4 words) makes them the
        whole matrix's.  The selection is then replicated -- kernels.auror_select gives the same flags on every rank -- and
        the sum of the kept rows over their count is local to the columns.  Returns this rank's columns (gather=True: the
        whole vector)."""
        import torch
        if alpha is None:
            raise ValueError('auror: alpha has no default')
        n = g_local.shape[0]
        votes, bad, counts = self.kernels.auror_votes(g_local, alpha, max_iter=max_iter)
        packed = torch.cat([votes.reshape(-1), bad.reshape(-1).to(torch.int64), counts.reshape(-1)])
        self._all_reduce('allreduce_auror_votes', packed)
        votes, bad, counts = packed[:n], (packed[n:2 * n] != 0).to(torch.int32), packed[2 * n:]
        kept, info = self.kernels.auror_select(votes, bad, counts, g_local, tau=tau)
        weights = (kept != 0).to(torch.float64)
        v = self.kernels.scaled_rows_sum(g_local, weights, weights.sum().reshape(1))
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        return out, dict(info, kept_rows=torch.nonzero(kept).reshape(-1).cpu().numpy(), votes=votes.cpu().numpy())

    def foolsgold(self, g_local, users_count=None, corrupted_count=None, history=None, columns=None, column_offset=0, kappa=1.0,
                  normalise='count', gather=False, total_columns=None, return_info=False):
        """FoolsGold (defences.foolsgold's contract), columns layout: every rank holds all rows over its own columns,
        `column_offset` being the global number of its first column and `total_columns` the full D (needed beyond one rank).
        Every rank keeps the history of ITS OWN columns: `history` is its device-resident float32 matrix of n x (the columns of
        the global window `columns` that fall into its slice), added to in place; a rank the window misses passes None and
        contributes a zero Gram.  ONE all-reduce: the N x N fp64 Gram, the exchange AFA makes.  Everything after it is
        replicated -- kernels.foolsgold_weights gives the same weights and T on every rank -- or local to the columns: the
        weighted sum over T.  No new collective.  Returns this rank's columns (gather=True: the whole vector)."""
        import torch
        n, d_local = g_local.shape
        total = d_local if total_columns is None else int(total_columns)
        c0, c1 = (0, total) if columns is None else (int(columns[0]), int(columns[1]))
        column_offset = int(column_offset)
        if not 0 <= c0 < c1 <= total:
            raise ValueError('foolsgold: the window [%d, %d) lies outside the %d columns' % (c0, c1, total))
        lo, hi = max(c0, column_offset), min(c1, column_offset + d_local)
        if hi > lo:
            local = (lo - column_offset, hi - column_offset)
            if history is not None:
                self.kernels.rows_add(history, g_local, columns=local)
                gram = self.kernels.gram(history)
            else:
                gram = self.kernels.gram(g_local[:, local[0]:local[1]])
        else:
            gram = torch.zeros((n, n), dtype=torch.float64, device=g_local.device)
        self._all_reduce('allreduce_gram', gram)
        weights, info = self.kernels.foolsgold_weights(gram, g_local, kappa=kappa, normalise=normalise)
        divisor = torch.tensor([info['divisor']], dtype=torch.float64, device=g_local.device)     # (the weights stage's own T)
        v = self.kernels.scaled_rows_sum(g_local, weights, divisor)
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        return out, dict(info, weights=weights.cpu().numpy())

    def nnm(self, g_local, users_count, corrupted_count, return_neighbours=False):
        """Nearest-neighbour mixing, columns layout: the distances' one all-reduce and nothing more; the neighbour lists are
        then the same on every rank and every rank mixes its own columns.  Returns the local slice (n x local columns) of the
        mixed matrix: the input of a rule of this class on the same layout.  A clients layout is not offered."""
        dist_m = self.global_distances(g_local)
        neighbours, counts = self.kernels.nnm_neighbours(dist_m, int(users_count) - int(corrupted_count))
        mixed = self.kernels.nnm_mix(g_local, neighbours, counts)
        return (mixed, neighbours) if return_neighbours else mixed

    def bucketing(self, g_local, users_count, corrupted_count, s=2, perm=None, seed=0):
        """s-bucketing, columns layout: a bucket's mean is local to a column, so every rank makes the single-GPU call on its
        own slice; no collective.  EVERY RANK MUST PASS THE SAME `perm`, or the same `seed` (the shuffle is then
        bucketing_permutation(rows, seed), drawn on each host alike): the buckets are then the same clients on every rank.
        Returns the local slice (ceil(n / s) x local columns) of the bucketed matrix: the input of a rule of this class on the
        same layout, called with ceil(n / s) users and the corrupted count unchanged.  A clients layout is not offered."""
        from .engine import bucketing_permutation
        if perm is None:
            perm = bucketing_permutation(g_local.shape[0], seed)
        return self.kernels.bucket_means(g_local, s, perm)

    def geometric_median(self, g_local, nu=1e-6, max_iter=10, ftol=1e-6, gather=False, return_info=False,
                         total_columns=None):
        """The geometric median (smoothed Weiszfeld, Engine.geometric_median's contract), columns layout: every rank
        holds all rows over its own columns.  A rank's squared distances to z cover its columns: one all-reduce of N
        doubles per iteration makes them whole, and the objective, the stop and the weights are then the same on every
        rank.  One more all-reduce of N + 1 doubles first decides the finiteness fallback on all-reduced data."""
        import torch
        n = g_local.shape[0]
        dev = g_local.device
        z = self.kernels.no_defense(g_local)
        ex = torch.zeros(n + 1, dtype=torch.float64, device=dev)
        if not bool(torch.isfinite(z).all().item()):
            # (a rank whose columns are finite adds 0: the sum's finiteness is the other ranks')
            ex[:n] = self.kernels.row_sqdist(g_local, torch.zeros_like(z))
            ex[n] = 1.0
        self._all_reduce('allreduce_geomed_finite', ex)
        fallback = bool(ex[n].item() > 0)
        active = torch.isfinite(ex[:n]) if fallback else torch.ones(n, dtype=torch.bool, device=dev)
        excluded = int((~active).sum().item())
        if fallback:
            z = self.kernels.weighted_mean(g_local, active.to(torch.float64))

        def distances(z):
            sq = self.kernels.row_sqdist(g_local, z)
            self._all_reduce('allreduce_geomed_distances', sq)
            d = torch.sqrt(sq)
            return d, float(d[active].sum().item())

        iterations, objective, beta = 0, 0.0, None
        if excluded < n:
            d, objective = distances(z)
            for k in range(1, int(max_iter) + 1):
                beta = torch.where(active, 1.0 / torch.clamp(d, min=float(nu)), torch.zeros_like(d))
                z = self.kernels.weighted_mean(g_local, beta)
                d, f_new = distances(z)
                stop = abs(objective - f_new) <= float(ftol) * f_new
                objective, iterations = f_new, k
                if stop:
                    break
        out = self._maybe_gather(z, gather, total_columns)
        if not return_info:
            return out
        if beta is not None:
            weights = beta / beta.sum()
        elif excluded < n:
            weights = active.to(torch.float64) / float(n - excluded)
        else:
            weights = torch.zeros(n, dtype=torch.float64, device=dev)
        return out, {'iterations': iterations, 'objective': objective, 'excluded_rows': excluded, 'weights': weights}

    def centered_clip(self, g_local, tau=10.0, iters=3, start=None, gather=False, return_info=False, total_columns=None):
        """Centered clipping (Engine.centered_clip's contract), columns layout: every rank holds all rows over its own
        columns of G and of `start` (None: zeros).  A rank's squared distances to the centre cover its columns: one
        all-reduce of N doubles per iteration makes them whole -- `iters` in all --, the scales are then the same on every
        rank and the update is local to the columns."""
        import torch
        tau, iters = float(tau), int(iters)
        if not tau > 0.0 or iters < 0:
            raise ValueError('centered_clip: tau = %r must be > 0, iters = %r >= 0' % (tau, iters))
        n, d_local = g_local.shape
        dev = g_local.device
        v = torch.zeros(d_local, dtype=torch.float32, device=dev) if start is None else \
            torch.as_tensor(start, dtype=torch.float32, device=dev).reshape(-1).clone()
        scales = torch.ones(n, dtype=torch.float64, device=dev)
        clipped = excluded = 0
        for _ in range(iters):
            sq = self.kernels.row_sqdist(g_local, v)
            self._all_reduce('allreduce_cclip_distances', sq)
            d = torch.sqrt(sq)
            finite = torch.isfinite(d)
            over = finite & (d > tau)
            scales = torch.where(over, tau / d, torch.where(finite, torch.ones_like(d), torch.zeros_like(d)))
            v = self.kernels.clip_update(g_local, v, scales)
            if return_info:
                clipped, excluded = int(over.sum().item()), int((~finite).sum().item())
        out = self._maybe_gather(v, gather, total_columns)
        if not return_info:
            return out
        return out, {'clipped_rows': clipped, 'excluded_rows': excluded, 'scales': scales}

    def fltrust(self, g_local, root_local, gather=False, return_info=False):
        """FLTrust (Engine.fltrust's contract), columns layout: every rank holds all rows over its own columns of G and of
        the root gradient.  A rank's dot products, squared norms and root norm cover its columns: ONE all-reduce of 2 N + 1
        doubles makes them whole, the trust scores are then the same on every rank and the sum is local to the columns."""
        import torch
        n, d_local = g_local.shape
        dev = g_local.device
        root_local = torch.as_tensor(root_local, dtype=torch.float32, device=dev).reshape(-1).contiguous()
        p, q = self.kernels.row_dots(g_local, root_local)
        q0 = self.kernels.row_sqdist(root_local.reshape(1, -1), torch.zeros_like(root_local))
        pq = torch.cat([p, q, q0])
        self._all_reduce('allreduce_fltrust_dots', pq)
        p, q, q0 = pq[:n], pq[n:2 * n], pq[2 * n]
        # include/byzagg.h's order of operations, in fp64
        root_ok = bool((torch.isfinite(q0) & (q0 > 0)).item())
        finite = torch.isfinite(p) & torch.isfinite(q)
        usable = finite & (q > 0)
        norm = torch.sqrt(torch.where(usable, q, torch.ones_like(q)))
        root_norm = torch.sqrt(q0)
        c = p / (norm * root_norm)
        zero = torch.zeros_like(c)
        trust = torch.where(usable & (c > 0), c, zero) if root_ok else zero
        weights = torch.where(trust != 0, trust * (root_norm / norm), zero)
        total = trust.sum()
        out = self.kernels.scaled_rows_sum(g_local, weights, total.reshape(1))
        out = self._maybe_gather(out, gather)
        if not return_info:
            return out
        return out, {'trusted_rows': int((trust > 0).sum().item()), 'excluded_rows': int((~finite).sum().item()),
                     'root_ok': root_ok, 'trust_sum': float(total.item()), 'trust': trust, 'weights': weights}

    def signguard(self, g_local, column_offset=0, total_columns=None, frac=0.1, lower=0.1, upper=3.0, bandwidth=None,
                  n_samples=50, seed=0, window=None, sample=None, gather=False, return_info=False):
        """SignGuard (defences.signguard's contract), columns layout: every rank holds all rows over its own columns,
        `column_offset` being the global number of its first column and `total_columns` the full D (needed beyond one rank).
        Every rank draws the SAME global window and sample (signguard_window, signguard_sample, or `window` / `sample`) and
        counts the part of the window that falls into its slice -- possibly nothing.  ONE all-reduce of 4 N doubles (pos,
        zero, neg, q; a count is exact as a double) makes them whole, the selection is then the same on every rank and the
        sum is local to the columns."""
        import torch
        from .engine import signguard_sample, signguard_window
        n, d_local = g_local.shape
        if self.world > 1 and total_columns is None:
            raise ValueError('signguard() over several ranks needs total_columns')
        total = int(total_columns) if total_columns is not None else d_local
        c0, m = window if window is not None else signguard_window(total, frac, seed)
        c0, m, column_offset = int(c0), int(m), int(column_offset)
        if c0 < 0 or m < 1 or c0 + m > total:
            raise ValueError('signguard: the window (%d, %d) is outside the %d columns' % (c0, m, total))
        lo, hi = max(c0, column_offset), min(c0 + m, column_offset + d_local)
        local_len = max(0, hi - lo)
        local_start = lo - column_offset if local_len else 0
        if sample is None and not (bandwidth is not None and float(bandwidth) > 0.0):
            sample = signguard_sample(n, n_samples, seed)
        pos, zero, neg, q = self.kernels.row_signs(g_local, local_start, local_len)
        pznq = torch.cat([torch.as_tensor(v, device=g_local.device).to(torch.float64).reshape(-1) for v in (pos, zero, neg, q)])
        self._all_reduce('allreduce_signguard_census', pznq)
        pos, zero, neg = (pznq[k * n:(k + 1) * n].to(torch.int64) for k in range(3))
        sel = self.kernels.signguard_select(pos, zero, neg, pznq[3 * n:], m, lower=lower, upper=upper, bandwidth=bandwidth,
                                            sample=sample)
        out = self.kernels.scaled_rows_sum(g_local, sel['weights'], sel['mk'][1:2])
        out = self._maybe_gather(out, gather, total_columns)
        if not return_info:
            return out
        info = self.kernels.engine.signguard_info() if hasattr(self.kernels, 'engine') else {}
        info.update(keep=sel['keep'], weights=sel['weights'], labels=sel['labels'], window=(c0, m))
        return out, info

    def dnc(self, g_local, users_count, corrupted_count, niters=1, filter_frac=1.0, sub_dim=10000, power_iters=32, seed=0,
            columns=None, gather=False, return_index=False, total_columns=None):
        """DnC (defences.dnc's contract), columns layout: every rank draws the SAME global sample (`dnc_columns(D, sub_dim,
        niters, seed)`, or `columns`) and keeps the part that falls into its own slice -- possibly nothing.  Column means and
        C^T u are local; the activity flags, the diagonal and every product are n-vectors summed over the ranks:
        niters * (power_iters + 3) all-reduces of n doubles, whatever the data.  The selection is the same on every rank,
        the mean is taken on the local columns.  total_columns (the full D) is needed beyond one rank."""
        from .engine import dnc_columns
        n, d_local = g_local.shape
        if self.world > 1 and total_columns is None:
            raise ValueError('dnc() over several ranks needs total_columns')
        total = int(total_columns) if total_columns is not None else int(d_local)
        lo, hi = self.column_slices(total)[self.rank] if self.world > 1 else (0, total)
        assert hi - lo == d_local, (lo, hi, d_local)
        if columns is None:
            columns = dnc_columns(total, sub_dim, niters, seed)
        columns = np.asarray(columns, dtype=np.int64)
        columns = columns.reshape(1, -1) if columns.ndim == 1 else columns
        if columns.min() < 0 or columns.max() >= total or (np.diff(columns, axis=1) <= 0).any():
            raise ValueError('column lists must be in [0, %d) and strictly ascending' % total)
        local = [row[(row >= lo) & (row < hi)] - lo for row in columns]
        remove_count = min(n - 1, int(filter_frac * corrupted_count))
        reduce = (lambda t: self._all_reduce('allreduce_dnc', t)) if self._collective() else None
        out, good = self.kernels.dnc(g_local, remove_count, local, columns.shape[1], power_iters=power_iters,
                                     all_reduce=reduce, return_selection=True)
        if return_index:
            return good
        return self._maybe_gather(out, gather, total_columns)

    # ---- defences.py, clients layout ----------------------------------------------------------------------------------
    def _row_owner(self, rows_per_rank):
        offsets = np.concatenate([[0], np.cumsum(rows_per_rank)]).astype(np.int64)
        return offsets

    def krum_clients(self, rows_local, rows_per_rank, users_count, corrupted_count, return_index=False):
        """Krum over client-sharded rows: distances by all-gather, replicated selection, the winner's row broadcast
        by its owner.  Returns the full D-vector on every rank."""
        if not return_index:
            assert users_count >= 2 * corrupted_count + 1, (
                'users_count>=2*corrupted_count + 3', users_count, corrupted_count)
        dist_m = self.client_distances(rows_local, rows_per_rank)
        index = int(self.kernels.krum_select(dist_m, users_count, corrupted_count))
        if return_index:
            return index
        offsets = self._row_owner(rows_per_rank)
        total = int(offsets[-1])
        row = index if index >= 0 else total + index       # numpy's G[-1]
        owner = int(np.searchsorted(offsets, row, side='right') - 1)
        import torch
        out = torch.empty(rows_local.shape[1], dtype=rows_local.dtype, device=rows_local.device)
        if owner == self.rank:
            out.copy_(rows_local[row - int(offsets[owner])])
        if self._collective():
            src = self.dist.get_global_rank(self.group, owner) if self.group is not None else owner
            self._timed('broadcast_row', out.numel() * out.element_size(), out,
                        lambda: self.dist.broadcast(out, src=src, group=self.group))
        return out

    def bulyan_clients(self, rows_local, rows_per_rank, users_count, corrupted_count, return_selection=False):
        """Bulyan over client-sharded rows (north_star's flow): all-gather distances, replicated selection loop, the
        theta selected rows re-sharded to column slices, median-window mean per slice, all-gather of the D-vector."""
        assert users_count >= 4 * corrupted_count + 3
        dist_m = self.client_distances(rows_local, rows_per_rank)
        selection = np.asarray(self.kernels.bulyan_select(dist_m, users_count, corrupted_count), dtype=np.int64)
        cols, row_index = self.reshard_rows_to_columns(rows_local, rows_per_rank, selection)
        out = self.kernels.trimmed_mean(cols, 2 * corrupted_count, row_index=row_index)
        out = self._maybe_gather(out, True, total=rows_local.shape[1])
        return (out, selection.astype(np.int32)) if return_selection else out

    def multi_krum_clients(self, rows_local, rows_per_rank, users_count, corrupted_count, m=None, return_selection=False):
        """Multi-Krum over client-sharded rows: all-gather distances, replicated selection, the selected rows (ascending)
        re-sharded to column slices, the row-list mean per slice, all-gather of the D-vector."""
        assert users_count >= 2 * corrupted_count + 1, (
            'users_count>=2*corrupted_count + 3', users_count, corrupted_count)
        dist_m = self.client_distances(rows_local, rows_per_rank)
        selection = np.asarray(self.kernels.multi_krum_select(dist_m, users_count, corrupted_count, m), dtype=np.int32)
        rows = np.sort(selection)
        cols, row_index = self.reshard_rows_to_columns(rows_local, rows_per_rank, rows)
        out = self.kernels.mean_rows(cols, np.arange(len(rows), dtype=np.int32) if row_index is None else row_index)
        out = self._maybe_gather(out, True, total=rows_local.shape[1])
        return (out, selection) if return_selection else out

    # ---- malicious.py --------------------------------------------------------------------------------------------------
    def drift_attack(self, g_local, n_malicious, num_std, write_back=True, gather=False, total_columns=None):
        """columns layout.  Rows 0..m-1 are the malicious clients (reference main.py:28); per column, no exchange."""
        drift, mean, std = self.kernels.drift(g_local[:n_malicious], num_std, write_back=write_back)
        return self._maybe_gather(drift, gather, total_columns), mean, std

    def minmax_attack(self, g_local, n_malicious, kind='minmax', perturbation='std', partial=False, return_info=False):
        """The Min-Max / Min-Sum attacks, columns layout, in place on rows 0..m-1 of this rank's slice.  The statistics, the
        perturbation and the fill are local to a column; a_i, b_i and c are sums over the columns: ONE all-reduce of 2 r + 1
        doubles (r: the known rows), with 'unit' one more of 1 double (|mu|^2) before it; Min-Max also takes the sharded
        distances' all-reduces (the Gram, the near-duplicate pairs).  Every rank solves the same gamma.  The clients layout is
        NOT offered: the moments of one client's row need every column of it on one rank, and mu needs every client's row."""
        reduce = (lambda t: self._all_reduce('allreduce_minmax', t)) if self._collective() else None
        return self.kernels.minmax_attack(g_local, n_malicious, kind=kind, perturbation=perturbation, partial=partial,
                                          all_reduce=reduce, return_info=return_info)

    def drift_attack_clients(self, rows_local, rows_per_rank, n_malicious, num_std, write_back=True):
        """clients layout.  The malicious rows 0..m-1 sit on the first ranks.  numpy's mean / var add in row order
        (malicious.py:18-19), so per column the additions are ONE chain through those ranks: each continues the running sums of
        the rank before it over its own malicious rows (`column_chain`: a point-to-point hop of D floats), the last holder
        ends the chain (`column_finish`) and broadcasts -- first the mean (the squared deviations need it), then std and the
        drifted vector.  Bit for bit what the unsharded attack returns (rounds 1-4 combined per-rank (sum, sum of squares) in
        fp64: 1e-6 close).  The drifted vector is written into every local malicious row.  Returns (drift, mean, std) as full
        D-vectors on every rank."""
        import torch
        if n_malicious <= 0:
            raise ValueError('drift_attack_clients: no malicious rows')
        offsets = self._row_owner(rows_per_rank)
        first = int(offsets[self.rank])
        m_local = int(min(max(n_malicious - first, 0), rows_per_rank[self.rank]))
        holders = [r for r in range(self.world)
                   if min(max(n_malicious - int(offsets[r]), 0), rows_per_rank[r]) > 0]
        last = holders[-1]
        d = rows_local.shape[1]
        where = holders.index(self.rank) if self.rank in holders else -1

        def peer(r):
            """torch.distributed addresses send / recv / broadcast by GLOBAL rank even when a group is given."""
            return self.dist.get_global_rank(self.group, r) if self.group is not None else r

        def walk(mean):
            """My link of one walk over the malicious rows; the total on the last holder."""
            if where < 0:
                return None
            carry = None
            if where > 0:
                carry = torch.empty(d, dtype=torch.float32, device=rows_local.device)
                self._timed('attack_chain_hop', 4 * d, carry, lambda: self.dist.recv(carry, src=peer(holders[where - 1]), group=self.group))
            total = self.kernels.column_chain(rows_local[:m_local], carry=carry, mean=mean)
            if where + 1 < len(holders):
                self._timed('attack_chain_hop', 4 * d, total, lambda: self.dist.send(total, dst=peer(holders[where + 1]), group=self.group),
                            count=False)
            return total

        total = walk(None)
        mean = (self.kernels.column_finish(n_malicious, num_std, sum=total) if self.rank == last
                else torch.empty(d, dtype=torch.float32, device=rows_local.device))
        if self._collective():
            self._timed('broadcast_attack_mean', 4 * d, mean, lambda: self.dist.broadcast(mean, src=peer(last), group=self.group))
        squares = walk(mean)
        if self.rank == last:
            std, drift = self.kernels.column_finish(n_malicious, num_std, sumsq=squares, mean=mean)
            both = torch.stack([std, drift])
        else:
            both = torch.empty((2, d), dtype=torch.float32, device=rows_local.device)
        if self._collective():
            self._timed('broadcast_attack_vector', 8 * d, both, lambda: self.dist.broadcast(both, src=peer(last), group=self.group))
        std, drift = both[0], both[1]
        if write_back and m_local > 0:
            rows_local[:m_local] = drift
        return drift, mean, std

    # ---- layout conversion ---------------------------------------------------------------------------------------------
    def column_slices(self, n_cols):
        """Column range owned by every rank: contiguous, sizes differ by at most one."""
        base, extra = divmod(n_cols, self.world)
        bounds, start = [], 0
        for r in range(self.world):
            stop = start + base + (1 if r < extra else 0)
            bounds.append((start, stop))
            start = stop
        return bounds

    def _exchange(self, name, blocks_out, blocks_in):
        """Personalised exchange: blocks_out[p] goes to rank p, blocks_in[p] is filled from rank p (point-to-point over
        the xGMI full mesh: all links busy, where a ring would be bound by one 153 GB/s link)."""
        ops = []
        nbytes = 0
        landed = []    # (contiguous landing buffer, strided destination): a block of a pitch-padded matrix is not contiguous
        for peer in range(self.world):
            if peer == self.rank and not self.always_collective:
                continue        # (BYZ_FORCE_COLLECTIVES=1: the rank's own block goes through RCCL too, send-to-self)
            global_peer = self.dist.get_global_rank(self.group, peer) if self.group is not None else peer
            if blocks_out[peer].numel():
                ops.append(self.dist.P2POp(self.dist.isend, blocks_out[peer], global_peer, group=self.group))
            if blocks_in[peer].numel():
                dst = blocks_in[peer]
                if not dst.is_contiguous():
                    dst = dst.new_empty(dst.shape)
                    landed.append((dst, blocks_in[peer]))
                ops.append(self.dist.P2POp(self.dist.irecv, dst, global_peer, group=self.group))
                nbytes += dst.numel() * dst.element_size()
        if not ops:
            return

        def run():
            for req in self.dist.batch_isend_irecv(ops):
                req.wait()
            for buf, dst in landed:
                dst.copy_(buf)
        self._timed(name, nbytes, blocks_in[(self.rank + 1) % self.world], run)

    def reshard_clients_to_columns(self, rows_local, rows_per_rank):
        """client-sharded (rows_local: my rows x D) -> column-sharded (all rows x my columns).

        `rows_per_rank[r]` is the number of clients rank r holds.  One personalised exchange: point-to-point
        sends of (my rows) x (peer's columns); the received blocks are stacked in rank order.
        """
        all_rows = np.arange(int(sum(rows_per_rank)), dtype=np.int64)
        cols, _ = self.reshard_rows_to_columns(rows_local, rows_per_rank, all_rows, name='reshard_clients_to_columns')
        return cols

    def reshard_rows_to_columns(self, rows_local, rows_per_rank, wanted_rows, name='reshard_selected_rows'):
        """The rows `wanted_rows` (global indices, any order, e.g. Bulyan's selection) as a column-sharded matrix.

        Returns (cols, row_index): `cols` is (len(wanted_rows), my columns), stacked by owning rank; `row_index[s]` is
        the row of `cols` that holds wanted_rows[s] (None when the stacking order already is the wanted order), so that
        `trimmed_mean(cols, ..., row_index=row_index)` sees the rows in the caller's order (defences.py:70)."""
        import torch
        wanted_rows = np.asarray(wanted_rows, dtype=np.int64)
        offsets = self._row_owner(rows_per_rank)
        owner = np.searchsorted(offsets, wanted_rows, side='right') - 1
        n_cols = rows_local.shape[1]
        bounds = self.column_slices(n_cols)
        lo, hi = bounds[self.rank]
        counts = [int(np.sum(owner == r)) for r in range(self.world)]
        starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        # position of wanted_rows[s] inside its owner's block = its rank among that owner's wanted rows, in wanted order
        within = np.zeros(len(wanted_rows), dtype=np.int64)
        for r in range(self.world):
            mask = owner == r
            within[mask] = np.arange(counts[r])
        row_index = (starts[owner] + within).astype(np.int32)
        mine = wanted_rows[owner == self.rank] - offsets[self.rank]
        device = rows_local.device
        mine_t = torch.from_numpy(mine).to(device)
        # the leading dimension is padded to a multiple of four floats: slice widths differ by one between ranks, and a
        # 16-byte-aligned row pitch is what lets every rank's kernels take the same (LDS-DMA, vector-load) paths
        pitch = -(-(hi - lo) // 4) * 4
        out = torch.empty((len(wanted_rows), pitch), dtype=rows_local.dtype, device=device)[:, :hi - lo]
        all_of_mine = len(mine) == rows_local.shape[0] and np.array_equal(mine, np.arange(rows_local.shape[0]))

        def block_for(p):
            """My wanted rows x rank p's columns, contiguous: ONE gather per peer straight out of the caller's matrix (the
            first version gathered the rows with all D columns and then cut every peer's block out of that copy: twice the
            memory -- 83 + 83 GB next to a 160 GB matrix at configs[3] on one rank)."""
            cols = rows_local[:, bounds[p][0]:bounds[p][1]]
            return cols.contiguous() if all_of_mine else cols.index_select(0, mine_t)
        blocks_in = [out[int(starts[p]):int(starts[p + 1])] for p in range(self.world)]
        through_rccl = self.always_collective          # the rank's own block as a send-to-self (tests the P2P path on one GPU)
        if not through_rccl:
            blocks_in[self.rank].copy_(rows_local[:, lo:hi] if all_of_mine else block_for(self.rank))
        if self.world > 1 or through_rccl:
            blocks_out = [block_for(p) if (p != self.rank or through_rccl) else rows_local[:0] for p in range(self.world)]
            self._exchange(name, blocks_out, blocks_in)
        plain = np.array_equal(row_index, np.arange(len(wanted_rows)))
        return out, (None if plain else row_index)

    def _maybe_gather(self, local_vec, gather, total=None):
        """All-gather of the column-sharded D-vector.  `total` (the full D) lets every rank compute every slice length;
        without it the lengths are exchanged first."""
        if not gather or not self._collective():
            return local_vec
        import torch
        if total is not None:
            lengths = [b - a for a, b in self.column_slices(int(total))]
            assert lengths[self.rank] == local_vec.shape[0]
        else:
            sizes = torch.tensor([local_vec.shape[0]], device=local_vec.device, dtype=torch.int64)
            all_sizes = [torch.zeros_like(sizes) for _ in range(self.world)]
            self.dist.all_gather(all_sizes, sizes, group=self.group)
            lengths = [int(s.item()) for s in all_sizes]
        width = max(lengths)
        padded = local_vec
        if local_vec.shape[0] != width:
            padded = torch.zeros(width, dtype=local_vec.dtype, device=local_vec.device)
            padded[:local_vec.shape[0]] = local_vec
        flat = torch.empty(width * self.world, dtype=local_vec.dtype, device=local_vec.device)
        self._timed('allgather_output', (self.world - 1) * width * local_vec.element_size(), padded,
                    lambda: self.dist.all_gather_into_tensor(flat, padded.contiguous(), group=self.group))
        if all(n == width for n in lengths):
            return flat
        return torch.cat([flat[p * width:p * width + n] for p, n in enumerate(lengths)])
