"""Segmentation of new data with a saved model (model_io.py): the second half of a segmentation tool's workflow.

`phyloHMRF.from_model(path, observation, len_vec, edge_list_1, **runtime)` builds the blocks and row tiles exactly as the
constructor does (it IS the constructor, with the model's K, S, tree, beta, beta1, estimate_type, num_neighbor, min_covar
and solver tolerance) and then puts the saved Gaussians in place: no k-means, no M-step, no checkpoint.
`model.segment(want_entropy=False)` runs per region
  1. the emission under the saved means_ / _covars_;
  2. a COLD solve from argmax_k logprob (init_mode 1) with the model's beta and tolerance -- no warm start exists for data
     the model has not seen, and a cold start depends on nothing but the model and the data, so the state numbers mean
     the same in every run;
  3. the per-node posterior summary (phmrf_posterior_summary: conf = posterior of the called state, top = the most probable
     state, optionally the entropy), 9 bytes per node to the host instead of K doubles.
Whole blocks run concurrently on the model's block runner; row tiles of split blocks through the Conductor, each tile from
the argmax of its own stored rows.  With several ranks every output position is written by exactly one rank, and the
outputs are gathered with the byte all-reduce (conf and entropy as their bit patterns) and the energies with the f64 one.
"""
import time

import numpy as np

from .model_io import check_observation, load_model

_FIT_ONLY = ("edge_list", "branch_list", "cons_param", "beta", "beta1", "initial_mode", "initial_weight", "initial_weight1",
             "initial_magnitude", "observation", "edge_list_1", "len_vec", "n_samples", "n_features", "n_components",
             "estimate_type", "min_covar", "num_neighbor", "checkpoint_path", "resume_from")


def from_model(cls, model, observation, len_vec, edge_list_1, **runtime):
    """model: a path or a model_io.Model.  runtime: the constructor's placement options (block_threads, split_above,
    tile_parts, device_graph, world, rank, reducer, block_factory, quiet, solver_opts overrides)."""
    m = load_model(model) if isinstance(model, str) else model
    check_observation(m, observation)                         # (before anything touches the GPU)
    bad = sorted(set(runtime) & set(_FIT_ONLY))
    if bad:
        raise ValueError("from_model takes %s from the model file, not as options" % ", ".join(bad))
    X = np.asarray(observation)
    solver_opts = dict(energy_tol_ppb=int(m.energy_tol_ppb))
    solver_opts.update(runtime.pop("solver_opts", None) or {})
    branch = m.branch_list.tolist() if m.branch_list is not None else [1.0] * len(m.edge_list)
    obj = cls(n_samples=X.shape[0], n_features=int(m.S), edge_list=m.edge_list.tolist(), branch_list=branch, cons_param=1.0,
              beta=float(m.beta), beta1=float(m.beta1), initial_mode=0, initial_weight=0.0, initial_weight1=0.0,
              initial_magnitude=1.0, observation=X, edge_list_1=edge_list_1, len_vec=len_vec, n_components=int(m.K),
              estimate_type=int(m.estimate_type), min_covar=float(m.min_covar), num_neighbor=int(m.num_neighbor),
              solver_opts=solver_opts, mstep_workers=0, **runtime)
    obj.means_, obj._covars_ = m.means_.copy(), m._covars_.copy()
    obj.params_vec, obj.params_vec1 = m.params_vec.copy(), m.params_vec1.copy()
    obj.model_file = m
    return obj


def segment(model, want_entropy=False):
    """-> dict(state_vec float64 [n] in global order, conf float32 [n], top uint8 [n], entropy float32 [n] or None,
    energy float64 [regions] (phmrf_mrf_energy of the labelling), timing {stage: ms summed over this rank's regions})"""
    n, R = int(model.n_samples), len(model.len_vec)
    beta, et = float(model.beta), int(model.estimate_type)
    means, covars = model.means_, model._covars_
    opts = dict(model.solver_opts, init_mode=1, coarse_start=0)
    labels = np.zeros(n, dtype=np.uint8)
    conf = np.zeros(n, dtype=np.float32)
    top = np.zeros(n, dtype=np.uint8)
    ent = np.zeros(n, dtype=np.float32) if want_entropy else None
    energy = np.zeros(R, dtype=np.float64)
    timing = dict(emission=0.0, solve=0.0, summary=0.0)

    def put(b, out, own_local, region):
        c, t, e = b.posterior_summary(beta, et, want_entropy)
        lo = own_local.start - b.owned[0]
        sl = slice(lo, lo + (out.stop - out.start))
        labels[out] = b.get_labels()[own_local]
        conf[out], top[out] = c[sl], t[sl]
        if want_entropy:
            ent[out] = e[sl]
        energy[region] += b.energy(beta)[0]

    def whole(r):
        b = model.blocks[r]
        t0 = time.perf_counter()
        b.emission(means, covars)
        b.sync()
        t1 = time.perf_counter()
        b.solve_fast(beta, **opts)
        t2 = time.perf_counter()
        s1, s2 = model.len_vec[r][1], model.len_vec[r][2]
        put(b, slice(s1, s2), slice(0, s2 - s1), r)
        return t1 - t0, t2 - t1, time.perf_counter() - t2

    by_size = sorted(model.my_regions, key=lambda r: -int(model.len_vec[r][0]))
    pending = model.runner.start(whole, by_size)
    tiled = dict(emission=0.0, summary=0.0)
    if model.conductor.groups:
        def prepare(tl):
            t0 = time.perf_counter()
            tl.b.emission(means, covars)
            tl.b.sync()
            tiled["emission"] += time.perf_counter() - t0

        region_of = {id(tl): g.block_id for g in model.conductor.groups for tl in g.local.values()}

        def finish(tl):
            t0 = time.perf_counter()
            r = region_of[id(tl)]
            s1 = model.len_vec[r][1]
            g = tl.owned_global_slice()
            put(tl.b, slice(s1 + g.start, s1 + g.stop), tl.owned_local_slice(), r)
            tiled["summary"] += time.perf_counter() - t0

        t0 = time.perf_counter()
        model.conductor.solve(beta, opts, prepare=prepare, finish=finish)
        timing["solve"] += time.perf_counter() - t0 - tiled["emission"] - tiled["summary"]
        timing["emission"] += tiled["emission"]
        timing["summary"] += tiled["summary"]
    for te, ts, tm in pending.results():
        timing["emission"] += te
        timing["solve"] += ts
        timing["summary"] += tm
    if model.world > 1:
        t0 = time.perf_counter()
        red = model.reducer
        labels = red.allreduce_bytes(labels)
        top = red.allreduce_bytes(top)
        conf = red.allreduce_bytes(conf.view(np.uint8)).view(np.float32)
        if want_entropy:
            ent = red.allreduce_bytes(ent.view(np.uint8)).view(np.float32)
        energy = red.allreduce(energy)
        timing["gather"] = time.perf_counter() - t0
    return dict(state_vec=labels.astype(np.float64), conf=conf, top=top, entropy=ent, energy=energy,
                timing={k: 1e3 * v for k, v in timing.items()})
