#!/usr/bin/env python3
"""Command line of the reference (`python phylo_hmrf.py -n K --chromvec 21,22 --miter M ...`, README.md:7-51;
parse_args / run, phylo_hmrf.py:1531-1760) driving the MI355X E-step.

Same flags, same defaults as the reference CODE (which differ from its README: --cons_param 1, --beta1 0.5,
--num_neighbor 8, --estimate_type 0; phylo_hmrf.py:1541,1552,1553,1556), same cache files
(data.<res>Kb.observed.<run>.npy, edgelist.<res>Kb.observed.<run>.npy, lenvec.<res>Kb.observed.<run>.txt,
phylo_hmrf.py:1676-1704) and the same output `estimate_ou_<run>_<lambda0>_<K>.mat` with the fields
state_vec, len_vec, params_vec1, params_vec2, iter_id1, iter_id2, cost_vec (:1743-1748).

Raw input (edge.1.txt, branch_length.1.txt, species_name.1.txt, path_list.txt, <ref>.chrom.sizes, chr<c>.synteny.txt and
the species' chr<c>.<res>K.txt contact files under --root_path, README.md:53-75) is pre-processed on the host by
phylo_hmrf_amd/preprocess.py, a restatement of utility.load_data_chromosome2 pinned on the reference's own loader
(tests/test_preprocess.py); --filter_mode 0 uses the build's Perona-Malik restatement of medpy's filter (medpy is not
installed: parity unpinned for that one function), --filter_mode 1 its restatement of skimage's bilateral filter
(scikit-image is not installed either: parity unpinned likewise).
--synthetic N instead generates a seeded multi-species block in the same cache format.
"""
from __future__ import print_function

import os
import sys
import time
from optparse import OptionParser

import numpy as np
import scipy.io

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def parse_args(argv=None):
    parser = OptionParser(usage="Phylo-HMRF state estimation", add_help_option=False)
    parser.add_option("-n", "--num_states", default="10", help="Set the number of states to estimate")
    parser.add_option("-f", "--chromosome", default="1", help="Chromosome name")
    parser.add_option("-l", "--length", default="one", help="Filename of length vectors")
    parser.add_option("-p", "--root_path", default=".", help="Root directory of the data files")
    parser.add_option("-m", "--multiple", default="true", help="Use multivariate data (true, default)")
    parser.add_option("-a", "--species_name", default="human", help="Species to estimate states")
    parser.add_option("-o", "--sort_states", default="false", help="Whether to sort the states")
    parser.add_option("-r", "--run_id", default="0", help="experiment id")
    parser.add_option("-c", "--cons_param", default="1", help="constraint parameter")
    parser.add_option("-t", "--method_mode", default="1", help="method_mode: 1: Phylo-HMRF")
    parser.add_option("-d", "--initial_mode", default="0", help="initial mode")
    parser.add_option("-i", "--initial_weight", default="0.3", help="initial weight 0 for initial parameters")
    parser.add_option("-k", "--initial_weight1", default="0.1", help="initial weight 1 for initial parameters")
    parser.add_option("-j", "--initial_magnitude", default="1", help="initial magnitude for initial parameters")
    parser.add_option("-s", "--simu_version", default="1", help="dataset version")
    parser.add_option("-u", "--position1", default="0", help="position1")
    parser.add_option("-v", "--position2", default="50000", help="position2")
    parser.add_option("-w", "--filter_sigma", default="0.25", help="sigma of filter")
    parser.add_option("-b", "--beta", default="1", help="beta")
    parser.add_option("--beta1", default="0.5", help="beta1")
    parser.add_option("--num_neighbor", default="8", help="number of neighbors")
    parser.add_option("--filter_mode", default="0", help="filter method")
    parser.add_option("-e", "--threshold", default="0.001", help="convergence threshold")
    parser.add_option("-g", "--estimate_type", default="0", help="the method used for estimating label")
    parser.add_option("-q", "--annotation", default="test", help="annotation of the filename")
    parser.add_option("--dtype", default="0", help="diagonal type")
    parser.add_option("--reload", default="0", help="reload existing processed data")
    parser.add_option("--quantile", default="1", help="whether to compute signal quantiles")
    parser.add_option("--miter", default="60", help="max number of iterations")
    parser.add_option("--resolution", default="50000", help="genomic bin size")
    parser.add_option("--ref_species", default="hg38", help="reference species id")
    parser.add_option("--chromvec", default="1", help="chromosomes to perform estimation")
    parser.add_option("--output", default=".", help="output directory to save files")
    # additions of this build
    parser.add_option("--synthetic", default="0", help="generate a seeded synthetic diagonal block of this side and "
                                                        "write it in the reference's cache format")
    parser.add_option("--seed", default="", help="random seed (default: non-deterministic like the reference)")
    parser.add_option("--quiet", default="0", help="1: suppress the per-iteration prints")
    parser.add_option("--init", default="minibatch", help="initial clustering: 'minibatch' = the reference's MiniBatchKMeans "
                      "(phylo_hmrf.py:234-238) for the centres, the assignment of all nodes and the per-cluster "
                      "statistics on the GPU; 'sklearn' = the reference's initialisation verbatim on the host; "
                      "'device' = Lloyd k-means on the GPU")
    parser.add_option("--warm_start", default="best", help="start of an E-step's labelling: 'local' = labels_local, the labels of "
                      "the iteration with the lowest cost so far, as the reference does (phylo_hmrf.py:479); 'best' (default) = "
                      "that or the previous E-step's labels, whichever has the lower energy under the new parameters")
    parser.add_option("--energy_tol_ppb", default="10000", help="the label solver of an E-step stops when a whole round lowers the "
                      "energy by less than this many parts per billion of it (default 10000 = 1e-5, the level at which two solves of "
                      "the same inputs differ; 1000 until round 6; 0 = to the exact fixed point, ~25x the E-step time)")
    parser.add_option("--checkpoint", default="", help="write an .npz checkpoint of the fit here after every "
                      "--checkpoint_every-th EM iteration (parameters, cost bookkeeping, labellings, random generator)")
    parser.add_option("--checkpoint_every", default="1", help="EM iterations between checkpoints")
    parser.add_option("--resume", default="", help="continue a fit from this checkpoint (same data, states and options)")
    parser.add_option("--save_model", default="", help="after the fit, write the model (tree, OU parameters, Gaussians, beta, "
                      "solver and preprocessing settings) to this .npz, for --segment")
    parser.add_option("--segment", default="", help="skip the fit: segment the data with the model saved at this path (cold "
                      "solve from argmax, per-bin confidence) and write segment_<run_id>_<K>.mat")
    parser.add_option("--ancestral", default="", help="with --segment: after the segmentation, reconstruct the contact map of "
                      "every internal tree node (posterior: weighted by the state posteriors; called: the called state's own "
                      "map) with its standard deviation, in the model's feature units, and write ancestral_<run_id>_<K>.npz")
    parser.add_option("--profile", default="0", help="1: after the .mat of a fit or of --segment is written, profile the states "
                      "of the state_vec it holds on the GPU (counts, exact quantiles, mean and sd per species, distance bands, "
                      "chromosome enrichment) and write profile_<run_id>_<K>.npz and .txt")
    parser.add_option("--profile_quantiles", default="0.003,0.25,0.5,0.75,0.997", help="--profile 1: up to 8 quantiles in [0, 1]")
    parser.add_option("--postprocess", default="", help="skip loading data and fitting: smooth the states of this "
                      "estimate_ou_*.mat or segment_*.mat (the reference's processing/*.m), write estimate_test<chrom>.ori.txt, "
                      ".smooth.txt and test<chrom>.region.txt in genome coordinates (--resolution) and smooth_<stem>.mat under --output")
    parser.add_option("--smooth_window", default="5", help="--postprocess: side of the neighbourhood window")
    parser.add_option("--smooth_area", default="-1", help="--postprocess: largest area of a small region (-1: the reference's "
                      "80, or 25 for a region less than 100 bins high)")
    parser.add_option("--smooth_iter", default="1", help="--postprocess: number of smoothing passes")
    parser.add_option("--filter_device", default="0", help="1: run the loader's smoothing filter (--filter_mode) on the GPU; "
                      "0 (default): on the host.  Not with --reload 1, --synthetic or --postprocess, which filter nothing")
    parser.add_option("--compare", default="", help="skip loading data and fitting: compare the states of this .mat with those "
                      "of --compare_with on the same regions (contingency table, agreement, ARI, NMI, differential domains); "
                      "writes compare_<A>__<B>.mat and compare_domains_<A>__<B>.txt in genome coordinates (--resolution) under "
                      "--output")
    parser.add_option("--compare_with", default="", help="--compare: the second .mat")
    parser.add_option("--compare_field", default="state_vec", help="--compare: state_vec or state_vec_smooth")
    parser.add_option("--compare_match", default="0", help="--compare: 1 = renumber the second map's states to the first's by "
                      "the best one-to-one assignment first (two fits of their own)")
    parser.add_option("--compare_min_conf", default="0", help="--compare: a differing bin pair counts only when both files' conf "
                      "reach this (0: every differing bin pair counts)")
    parser.add_option("--compare_area", default="-1", help="--compare: smallest area of a listed domain (-1: one more than the "
                      "smoothing's small-region area, 81, or 26 for a region less than 100 bins high)")
    parser.add_option("--domains", default="", help="skip loading data and fitting: list the domains of the states of this "
                      ".mat (the 8-connected same-state regions of every region's full matrix: box, area, boundary, distance "
                      "range) and count the edges between every pair of states; writes domains_<stem>.mat and "
                      "domains_<stem>.txt in genome coordinates (--resolution) under --output")
    parser.add_option("--domains_field", default="state_vec", help="--domains: state_vec or state_vec_smooth")
    parser.add_option("--domains_area", default="-1", help="--domains: smallest area of a listed domain (-1: as --compare_area)")
    parser.add_option("--render", default="", help="skip loading data and fitting: draw the states of this .mat, one PNG per "
                      "region of the region's full matrix reduced to at most --render_side pixels a side (a pixel takes the "
                      "state most of its bin pairs hold); writes render_<stem>_r<region>_chr<chrom>.png, render_<stem>.npz "
                      "and render_<stem>_legend.txt under --output")
    parser.add_option("--render_field", default="state_vec", help="--render: state_vec or state_vec_smooth")
    parser.add_option("--render_side", default="2048", help="--render: the largest side of an image in pixels (>= 1)")
    parser.add_option("--render_colors", default="", help="--render: a text file of R G B rows (0 .. 255), one per state, in "
                      "place of the built-in palette")
    parser.add_option("--render_outline", default="0", help="--render: 1 = draw the borders between states in black")
    parser.add_option("--render_conf", default="0", help="--render: 1 = fade every pixel towards white by the file's conf")
    parser.add_option("--render_mark", default="", help="--render: a compare_*.mat on the same regions; the bin pairs of its "
                      "differential domains (diff_vec == 2) are highlighted")
    parser.add_option("--tracks", default="", help="skip loading data and fitting: project the states of this .mat onto the "
                      "genome, per bin the state composition of the bin's row of the contact matrix within each window of "
                      "--tracks_dist; writes tracks_<stem>.npz and one tracks_<stem>_w<window>.txt per window in genome "
                      "coordinates (--resolution) under --output")
    parser.add_option("--tracks_field", default="state_vec", help="--tracks: state_vec or state_vec_smooth")
    parser.add_option("--tracks_dist", default="0-", help="--tracks: at most 8 windows of genomic distance in bp, lo-hi or lo- "
                      "(no upper limit), separated by commas; the default 0- is every distance")
    parser.add_option("--enrich", default="", help="skip loading data and fitting: count the states of this .mat between the "
                      "annotated classes of --enrich_bed (pairs of bins by class pair, inside one interval or not) against an "
                      "expectation matched by exact genomic distance; writes enrich_<stem>.npz and enrich_<stem>.txt under "
                      "--output (--resolution gives the bin size)")
    parser.add_option("--enrich_bed", default="", help="--enrich: the annotation, a text file of `chrom start stop name` lines "
                      "with at most 7 distinct names")
    parser.add_option("--enrich_field", default="state_vec", help="--enrich: state_vec or state_vec_smooth")
    parser.add_option("--enrich_dist", default="0-", help="--enrich: ONE window of genomic distance in bp, lo-hi or lo- (no upper "
                      "limit); the default 0- is every distance")
    parser.add_option("--enrich_segments", default="0", help="--enrich: 1 = every line of --enrich_bed is a segment of its own "
                      "(a TAD list): bin pairs inside one interval are counted apart from pairs across intervals")
    parser.add_option("--enrich_null", default="0", help="--enrich: 0 = off; N in 1 .. 10000 = a permutation null of N draws, every "
                      "draw a random circular shift of the annotation along every chromosome, recounted on the GPU with its "
                      "own distance-matched expectation; adds the null's tables, z-scores and p-values to enrich_<stem>.npz and "
                      "writes enrich_<stem>_null.txt")
    parser.add_option("--enrich_null_min", default="1000000", help="--enrich_null: the smallest shift in bp (at least one bin)")
    parser.add_option("--enrich_null_seed", default="0", help="--enrich_null: the seed of the shifts")
    parser.add_option("--pileup", default="", help="skip loading data and fitting: pile the states of this .mat up around the "
                      "anchors of --pileup_bed or the anchor pairs of --pileup_bedpe (the state counts per cell of a window of "
                      "+- --pileup_flank around every anchor, summed over the anchors of a name); writes pileup_<stem>.npz, "
                      "pileup_<stem>.txt and one pileup_<stem>_<name>.png per name under --output (--resolution gives the bin size)")
    parser.add_option("--pileup_bed", default="", help="--pileup: a BED file `chrom start stop [name [score [strand]]]` with at "
                      "most 8 distinct names; the piles are centred on the diagonal and flipped for strand -")
    parser.add_option("--pileup_bedpe", default="", help="--pileup: a BEDPE file `chrom1 start1 stop1 chrom2 start2 stop2 [name]`; "
                      "the piles are centred on the pairs of the two midpoints")
    parser.add_option("--pileup_field", default="state_vec", help="--pileup: state_vec or state_vec_smooth")
    parser.add_option("--pileup_flank", default="1000000", help="--pileup: the window reaches this many bp to either side of an "
                      "anchor (at most 64 bins)")
    parser.add_option("--pileup_shift", default="0", help="--pileup: also pile up controls, every anchor shifted by this many bp "
                      "(a whole number of bins) along the diagonal in both directions; 0: no controls")
    parser.add_option("--pileup_colors", default="", help="--pileup: a text file of R G B rows (0 .. 255), one per state, in "
                      "place of the built-in palette")
    parser.add_option("--consensus", default="", help="skip loading data and fitting: vote on the state maps of these .mat "
                      "files, A.mat,B.mat,... (2 .. 16 files on the same regions: repeated fits, or one model's segmentations of "
                      "several replicates); writes consensus_<stem of the first>_<M>.mat (the most voted state per bin pair, "
                      "the lowest on ties, with conf = the vote share: a state map every other mode reads), consensus_<...>.txt "
                      "and consensus_domains_<...>.txt under --output (--resolution gives the bin size)")
    parser.add_option("--consensus_field", default="state_vec", help="--consensus: state_vec or state_vec_smooth")
    parser.add_option("--consensus_match", default="0", help="--consensus: 1 = renumber the states of every later file to the "
                      "first file's by the assignment with the largest agreement (separate fits)")
    parser.add_option("--consensus_support", default="-1", help="--consensus: a bin pair is stable when this many files hold "
                      "its consensus state; -1: the strict majority")
    parser.add_option("--consensus_area", default="-1", help="--consensus: list the stable domains of at least this area in "
                      "bin pairs; -1: --domains_area's rule")
    parser.add_option("--query", default="", help="skip loading data and fitting: the state composition of this .mat inside every "
                      "interval of --query_bed (the bin pairs inside a TAD) or between the two intervals of every line of "
                      "--query_bedpe (a loop, a TAD pair, an enhancer-promoter pair): per line the state counts, the dominant state, "
                      "its share, the entropy and the mean confidence; writes query_<stem>.npz and query_<stem>.txt under "
                      "--output (--resolution gives the bin size)")
    parser.add_option("--query_bed", default="", help="--query: a BED file `chrom start stop [name]`; an interval takes every bin "
                      "it overlaps")
    parser.add_option("--query_bedpe", default="", help="--query: a BEDPE file `chrom1 start1 stop1 chrom2 start2 stop2 [name]`, "
                      "both ends on one chromosome")
    parser.add_option("--query_field", default="state_vec", help="--query: state_vec or state_vec_smooth")
    parser.add_option("--query_shift", default="0", help="--query: also count two controls per line, both intervals shifted by "
                      "this many bp (a whole number of bins) along the diagonal in either direction; 0: no controls")
    parser.add_option("--aggregate", default="", help="skip loading data and fitting: the rescaled pile-up of this .mat over the "
                      "intervals of --aggregate_bed (TAD or domain bodies) or the interval pairs of --aggregate_bedpe: every "
                      "feature is stretched or shrunk onto a grid of --aggregate_body cells with --aggregate_flank cells on either "
                      "side, and per grid cell the features vote with their dominant state; writes aggregate_<stem>.npz, "
                      "aggregate_<stem>.txt and one aggregate_<stem>_<name>.png per name under --output (--resolution gives the "
                      "bin size)")
    parser.add_option("--aggregate_bed", default="", help="--aggregate: a BED file `chrom start stop [name [score [strand]]]` with at "
                      "most 8 distinct names; an interval takes every bin it overlaps, strand - reverses the feature")
    parser.add_option("--aggregate_bedpe", default="", help="--aggregate: a BEDPE file `chrom1 start1 stop1 chrom2 start2 stop2 "
                      "[name]`, both ends on one chromosome")
    parser.add_option("--aggregate_field", default="state_vec", help="--aggregate: state_vec or state_vec_smooth")
    parser.add_option("--aggregate_body", default="32", help="--aggregate: the cells a feature's body is cut into, 1 .. 64")
    parser.add_option("--aggregate_flank", default="16", help="--aggregate: the cells on either side of the body, 0 .. 32; a flank "
                      "cell is as long as a body cell, so the flank scales with the feature")
    parser.add_option("--aggregate_shift", default="0", help="--aggregate: also pile up controls, every feature shifted by this many "
                      "bp (a whole number of bins) along the diagonal in either direction; 0: no controls")
    parser.add_option("--aggregate_min", default="0", help="--aggregate: leave out features (for a BEDPE line: ends) shorter than "
                      "this many bp")
    parser.add_option("--aggregate_colors", default="", help="--aggregate: a text file of R G B rows (0 .. 255), one per state, in "
                      "place of the built-in palette")
    parser.add_option("--regrid", default="", help="skip loading data and fitting: resample the states of this .mat, whose bins "
                      "are --regrid_from bp, onto bins of --resolution bp (every target bin pair takes the state that covers most "
                      "of it, the lowest on ties, by exact overlap areas over the chromosome's full matrix); writes "
                      "regrid_<stem>_<resolution>.mat (a state map every other mode reads, with conf = the vote share) and "
                      "regrid_<stem>_<resolution>.txt under --output")
    parser.add_option("--regrid_from", default="", help="--regrid: the bin size of the .mat in bp (required)")
    parser.add_option("--regrid_like", default="", help="--regrid: a .mat at --resolution whose len_vec gives the target regions "
                      "(copied as it is, so that --compare accepts the two files); default: the source's own regions on the new bins")
    parser.add_option("--regrid_field", default="state_vec", help="--regrid: state_vec or state_vec_smooth")
    parser.add_option("--regrid_cover", default="50", help="--regrid: a target bin pair is called when the source covers at least "
                      "this many percent of it, 0 .. 100 (0: any coverage); else it takes the state K, `uncovered`")
    parser.add_option("-h", "--help", action="help")
    opts, _ = parser.parse_args(argv)
    return opts


def cache_names(output_path, resolution, run_id, annot1="observed"):
    kb = int(resolution / 1000)
    return ("%s/data.%dKb.%s.%d.npy" % (output_path, kb, annot1, run_id),
            "%s/edgelist.%dKb.%s.%d.npy" % (output_path, kb, annot1, run_id),
            "%s/lenvec.%dKb.%s.%d.txt" % (output_path, kb, annot1, run_id))


def write_cache(output_path, resolution, run_id, samples, edge_list_vec, len_vec):
    """(several ranks: every one builds the same data, rank 0 writes the cache -- each file under a temporary name first and
    renamed when complete, so that no reader ever sees a truncated file)"""
    if int(os.environ.get("RANK", "0")) != 0:
        return
    f1, f2, f3 = cache_names(output_path, resolution, run_id)
    arr = np.empty(len(edge_list_vec), dtype=object)
    for i, e in enumerate(edge_list_vec):
        arr[i] = e
    with open(f1 + ".tmp", "wb") as fh:
        np.save(fh, samples)
    with open(f2 + ".tmp", "wb") as fh:
        np.save(fh, arr, allow_pickle=True)
    np.savetxt(f3 + ".tmp", np.asarray(len_vec), fmt="%d", delimiter="\t")
    for f in (f1, f2, f3):
        os.replace(f + ".tmp", f)


def init_process_group():
    """several GPUs (`python -m torch.distributed.run --nproc-per-node N phylo_hmrf.py ...`): the process group is set up FIRST
    -- before any data is loaded, so that a rank that fails early does not leave the others waiting in the rendezvous, and
    before anything touches the GPU.  -> (rank, world)"""
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world > 1:
        import torch
        import torch.distributed as dist
        if not dist.is_initialized():
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29519")
            backend = os.environ.get("PHMRF_DIST_BACKEND", "nccl")
            if backend == "nccl":
                local = 0 if os.environ.get("PHMRF_ONE_GPU") == "1" else int(os.environ.get("LOCAL_RANK", "0"))
                torch.cuda.set_device(local)
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))
            else:
                dist.init_process_group(backend, rank=rank, world_size=world)
    return rank, world


def all_ranks_agree(value):
    """rank 0's value on every rank (a decision about files must be ONE decision)"""
    if int(os.environ.get("WORLD_SIZE", "1")) <= 1:
        return value
    import torch.distributed as dist
    box = [value]
    dist.broadcast_object_list(box, src=0)
    return box[0]


def load_cache(output_path, resolution, run_id):
    f1, f2, f3 = cache_names(output_path, resolution, run_id)
    samples = np.load(f1)
    edge_list_vec = list(np.load(f2, allow_pickle=True))
    len_vec = np.atleast_2d(np.loadtxt(f3, dtype="int32", delimiter="\t"))
    return samples, len_vec, edge_list_vec


def synthetic_cache(N, S, K, num_neighbor, seed):
    """One N x N diagonal block in the reference's (samples, len_vec, edge_list_vec) form."""
    from phylo_hmrf_amd import synthetic
    from phylo_hmrf_amd.graph_host import grid_edges
    from phylo_hmrf_amd.tree import PhyloTree
    rng = np.random.default_rng(seed)
    tree = PhyloTree(synthetic.tree_for(S))
    params = synthetic.sample_ou_params(rng, tree, K)
    means, covars = tree.mean_cov(params)
    covars = covars + 1e-3 * np.eye(S)
    img = synthetic.label_image(rng, N, N, K)
    ii, jj = np.triu_indices(N)
    lab = img[ii, jj]
    L = np.linalg.cholesky(covars)
    X = np.maximum(means[lab] + np.einsum("nij,nj->ni", L[lab], rng.standard_normal((lab.shape[0], S))), 0.0)
    edges = grid_edges(X, N, N, True, num_neighbor)
    n = X.shape[0]
    len_vec = [[n, 0, n, N, N, 0, 0, 0, 1, 1]]        # utility.py:455-456, :528
    return X, len_vec, [edges], synthetic.tree_for(S)


PARSER_DEFAULTS = dict(num_states="10", resolution="50000", num_neighbor="8", filter_mode="0", filter_sigma="0.25", dtype="0")


def segment_settings(m, num_states, resolution, num_neighbor, filter_mode, filter_sigma, diagonal_type):
    """--segment: the run's K and feature settings from the model file.  A value that differs from the parser's default is
    an explicit one; if it also differs from the model's, the data would not be the model's features: ValueError."""
    given = dict(num_states=num_states, resolution=resolution, num_neighbor=num_neighbor, filter_mode=filter_mode,
                 filter_sigma=filter_sigma, dtype=diagonal_type)
    saved = dict(num_states=m.K, resolution=m.resolution, num_neighbor=m.num_neighbor, filter_mode=m.filter_mode,
                 filter_sigma=m.filter_sigma, dtype=m.diagonal_type)
    out = {}
    for k, v in given.items():
        model_v = saved[k]
        known = model_v is not None and np.isfinite(float(model_v)) and not (k != "filter_sigma" and int(model_v) == -1)
        explicit = str(v) != PARSER_DEFAULTS[k]
        if known and explicit and float(v) != float(model_v):
            raise ValueError("--%s %s differs from the model's %s (%s): segmenting needs the features the model was fitted on"
                             % (k, v, model_v, "--segment"))
        out[k] = str(model_v) if known else v
    return (out["num_states"], out["resolution"], out["num_neighbor"], out["filter_mode"], out["filter_sigma"], out["dtype"])


def check_ancestral(ancestral, segment, postprocess, regrid=""):
    """--ancestral posterior|called reconstructs on a segmentation's labels: only together with --segment"""
    if not ancestral:
        return
    if ancestral not in ("posterior", "called"):
        raise SystemExit("--ancestral must be posterior or called, not %r (it goes with --segment)" % (ancestral,))
    if postprocess:
        raise SystemExit("--ancestral cannot be combined with --postprocess, which loads no data: it goes with --segment")
    if regrid:
        raise SystemExit("--ancestral cannot be combined with --regrid, which loads no data: it goes with --segment")
    if not segment:
        raise SystemExit("--ancestral needs --segment: the ancestors are reconstructed with a saved model on the labels of "
                         "its segmentation")


def check_profile(profile, profile_quantiles, postprocess, compare, consensus="", query="", aggregate="", regrid=""):
    """--profile 1 needs the observations on the GPU: it goes with a fit or --segment -> the quantiles, or None when off"""
    if str(profile) not in ("0", "1"):
        raise SystemExit("--profile must be 0 or 1")
    if str(profile) == "0":
        return None
    for name, value in (("--postprocess", postprocess), ("--compare", compare), ("--consensus", consensus), ("--query", query),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--profile 1 cannot be combined with %s, which loads no data: the profile needs the observations"
                             % name)
    from phylo_hmrf_amd.profile import parse_quantiles
    try:
        return parse_quantiles(profile_quantiles)
    except ValueError as e:
        raise SystemExit("--profile_quantiles: %s" % e)


def write_profile(model, state_vec, quantiles, output_path, run_id, K, species, rank):
    """profile the written state_vec (a collective: every rank takes part, rank 0 writes)"""
    from phylo_hmrf_amd import profile as _profile
    start = time.time()
    prof = model.state_profile(quantiles=quantiles, state_vec=state_vec)
    print("profile use time: %s %s" % (time.time() - start, prof["timing"]))
    if rank == 0:
        stem = "%s/profile_%d_%d" % (output_path, run_id, K)
        _profile.save_npz(stem + ".npz", prof, species)
        _profile.save_txt(stem + ".txt", prof, species)


def check_compare(compare, compare_with, compare_field, compare_match, segment, postprocess, ancestral, save_model,
                  filter_device, consensus="", query="", aggregate="", regrid=""):
    """--compare A.mat --compare_with B.mat reads two finished state maps: it goes with nothing that loads data or fits"""
    if not compare and not compare_with:
        return
    if not compare or not compare_with:
        raise SystemExit("--compare and --compare_with go together: the two .mat files to compare")
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--ancestral", ancestral),
                        ("--save_model", save_model), ("--filter_device 1", str(filter_device) == "1"),
                        ("--consensus", consensus), ("--query", query),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--compare cannot be combined with %s: it loads no data and fits nothing" % name)
    if compare_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--compare_field must be state_vec or state_vec_smooth, not %r" % (compare_field,))
    if str(compare_match) not in ("0", "1"):
        raise SystemExit("--compare_match must be 0 or 1")


def check_domains(domains, domains_field, segment, postprocess, compare, ancestral, save_model, profile, filter_device,
                  consensus="", query="", aggregate="", regrid=""):
    """--domains FILE.mat reads one finished state map: it goes with nothing that loads data or fits"""
    if not domains:
        return
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--compare", compare),
                        ("--ancestral", ancestral), ("--save_model", save_model), ("--profile 1", str(profile) == "1"),
                        ("--filter_device 1", str(filter_device) == "1"), ("--consensus", consensus), ("--query", query),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--domains cannot be combined with %s: it loads no data and fits nothing" % name)
    if domains_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--domains_field must be state_vec or state_vec_smooth, not %r" % (domains_field,))


def check_render(render, render_field, render_side, render_outline, render_conf, segment, postprocess, compare, domains,
                 ancestral, save_model, profile, filter_device, consensus="", query="", aggregate="", regrid=""):
    """--render FILE.mat reads one finished state map: it goes with nothing that loads data or fits -> the side, or None"""
    if not render:
        return None
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--compare", compare), ("--domains", domains),
                        ("--ancestral", ancestral), ("--save_model", save_model), ("--profile 1", str(profile) == "1"),
                        ("--filter_device 1", str(filter_device) == "1"), ("--consensus", consensus), ("--query", query),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--render cannot be combined with %s: it loads no data and fits nothing" % name)
    if render_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--render_field must be state_vec or state_vec_smooth, not %r" % (render_field,))
    for name, value in (("--render_outline", render_outline), ("--render_conf", render_conf)):
        if str(value) not in ("0", "1"):
            raise SystemExit("%s must be 0 or 1" % name)
    try:
        side = int(render_side)
    except ValueError:
        side = 0
    if side < 1:
        raise SystemExit("--render_side must be an integer >= 1, not %r" % (render_side,))
    return side


def check_tracks(tracks, tracks_field, tracks_dist, resolution, render, segment, postprocess, compare, domains, ancestral,
                 save_model, profile, filter_device, consensus="", query="", aggregate="", regrid=""):
    """--tracks FILE.mat reads one finished state map: it goes with nothing that loads data or fits -> the windows in bins,
    or None"""
    if not tracks:
        return None
    for name, value in (("--render", render), ("--segment", segment), ("--postprocess", postprocess), ("--compare", compare),
                        ("--domains", domains), ("--ancestral", ancestral), ("--save_model", save_model),
                        ("--profile 1", str(profile) == "1"), ("--filter_device 1", str(filter_device) == "1"),
                        ("--consensus", consensus), ("--query", query),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--tracks cannot be combined with %s: it loads no data and fits nothing" % name)
    if tracks_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--tracks_field must be state_vec or state_vec_smooth, not %r" % (tracks_field,))
    from phylo_hmrf_amd.tracks import parse_windows
    try:
        return parse_windows(tracks_dist, int(resolution))
    except ValueError as e:
        raise SystemExit("--tracks_dist: %s" % e)


def check_enrich(enrich, enrich_bed, enrich_field, enrich_dist, enrich_segments, resolution, segment, postprocess, compare,
                 domains, render, tracks, ancestral, save_model, profile, filter_device, consensus="", query="", aggregate="", regrid=""):
    """--enrich FILE.mat --enrich_bed FILE reads one finished state map and an annotation: it goes with nothing that loads data
    or fits, and with no other reader of a state map -> the window (d_min, d_max) in bins, or None"""
    if not enrich:
        if enrich_bed:
            raise SystemExit("--enrich and --enrich_bed go together: the .mat and its annotation file")
        return None
    if not enrich_bed:
        raise SystemExit("--enrich and --enrich_bed go together: the .mat and its annotation file")
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--compare", compare), ("--domains", domains),
                        ("--render", render), ("--tracks", tracks), ("--ancestral", ancestral), ("--save_model", save_model),
                        ("--profile 1", str(profile) == "1"), ("--filter_device 1", str(filter_device) == "1"),
                        ("--consensus", consensus), ("--query", query),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--enrich cannot be combined with %s: it loads no data and fits nothing" % name)
    if enrich_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--enrich_field must be state_vec or state_vec_smooth, not %r" % (enrich_field,))
    if str(enrich_segments) not in ("0", "1"):
        raise SystemExit("--enrich_segments must be 0 or 1")
    from phylo_hmrf_amd.tracks import parse_windows
    try:
        wins = parse_windows(enrich_dist, int(resolution))
    except ValueError as e:
        raise SystemExit("--enrich_dist: %s" % e)
    if len(wins) != 1:
        raise SystemExit("--enrich_dist takes one window lo-hi or lo-, not %d" % len(wins))
    return wins[0]


def check_enrich_null(enrich, enrich_null="0", enrich_null_min="1000000", enrich_null_seed="0", resolution="50000"):
    """--enrich_null N, --enrich_null_min BP and --enrich_null_seed S go with --enrich -> (N, the smallest shift in bins, the
    seed); N = 0: no null.  (N 2 C C K < 2^26 is checked once the map and the annotation are read: enrich.check_null_size.)"""
    try:
        n, min_bp, seed = int(enrich_null), int(enrich_null_min), int(enrich_null_seed)
    except ValueError:
        raise SystemExit("--enrich_null, --enrich_null_min and --enrich_null_seed must be integers")
    if not enrich:
        if (n, min_bp, seed) != (0, 1000000, 0):
            raise SystemExit("--enrich_null, --enrich_null_min and --enrich_null_seed go with --enrich")
        return 0, 0, 0
    if not 0 <= n <= 10000:
        raise SystemExit("--enrich_null must be 0 (no null) or lie in 1 .. 10000, not %d" % n)
    if n == 0 and (min_bp, seed) != (1000000, 0):
        raise SystemExit("--enrich_null_min and --enrich_null_seed go with --enrich_null N")
    if min_bp < 0 or seed < 0:
        raise SystemExit("--enrich_null_min and --enrich_null_seed must be >= 0")
    return n, max(1, min_bp // int(resolution)), seed


def check_pileup(pileup, pileup_bed, pileup_bedpe, pileup_field, pileup_flank, pileup_shift, resolution, segment, postprocess,
                 compare, domains, render, tracks, enrich, ancestral, save_model, profile, filter_device, consensus="", query="", aggregate="",
                 regrid=""):
    """--pileup FILE.mat with --pileup_bed FILE or --pileup_bedpe FILE reads one finished state map and a list of anchors: it
    goes with nothing that loads data or fits, and with no other reader of a state map -> (the flank, the shift) in bins, or
    None"""
    if not pileup:
        if pileup_bed or pileup_bedpe:
            raise SystemExit("--pileup_bed and --pileup_bedpe go with --pileup: the .mat to pile up")
        return None
    if bool(pileup_bed) == bool(pileup_bedpe):
        raise SystemExit("--pileup takes its anchors from --pileup_bed or from --pileup_bedpe: exactly one of the two")
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--compare", compare), ("--domains", domains),
                        ("--render", render), ("--tracks", tracks), ("--enrich", enrich), ("--ancestral", ancestral),
                        ("--save_model", save_model), ("--profile 1", str(profile) == "1"),
                        ("--filter_device 1", str(filter_device) == "1"), ("--consensus", consensus), ("--query", query),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--pileup cannot be combined with %s: it loads no data and fits nothing" % name)
    if pileup_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--pileup_field must be state_vec or state_vec_smooth, not %r" % (pileup_field,))
    from phylo_hmrf_amd.pileup import check_bins
    try:
        return check_bins(int(resolution), int(pileup_flank), int(pileup_shift))
    except ValueError as e:
        raise SystemExit("--pileup with --pileup_flank %s and --pileup_shift %s: %s" % (pileup_flank, pileup_shift, e))


def check_consensus(consensus, consensus_field, consensus_match, consensus_support, consensus_area, segment, postprocess,
                    compare, domains, render, tracks, enrich, pileup, ancestral, save_model, profile, filter_device, query="", aggregate="",
                    regrid=""):
    """--consensus A.mat,B.mat,... reads finished state maps of the same regions: it goes with nothing that loads data or
    fits, and with no other reader of a state map -> (the files, min_support or None, min_area or None), or None"""
    if not consensus:
        return None
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--compare", compare), ("--domains", domains),
                        ("--render", render), ("--tracks", tracks), ("--enrich", enrich), ("--pileup", pileup),
                        ("--ancestral", ancestral), ("--save_model", save_model), ("--profile 1", str(profile) == "1"),
                        ("--filter_device 1", str(filter_device) == "1"), ("--query", query),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--consensus cannot be combined with %s: it loads no data and fits nothing" % name)
    from phylo_hmrf_amd.consensus import CONSENSUS_MAPS
    files = [f for f in str(consensus).split(",") if f]
    if not 2 <= len(files) <= CONSENSUS_MAPS:
        raise SystemExit("--consensus takes 2 .. %d .mat files separated by commas, not %d" % (CONSENSUS_MAPS, len(files)))
    if consensus_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--consensus_field must be state_vec or state_vec_smooth, not %r" % (consensus_field,))
    if str(consensus_match) not in ("0", "1"):
        raise SystemExit("--consensus_match must be 0 or 1")
    try:
        support, area = int(consensus_support), int(consensus_area)
    except ValueError:
        raise SystemExit("--consensus_support and --consensus_area must be integers")
    if support != -1 and not 1 <= support <= len(files):
        raise SystemExit("--consensus_support must be -1 (the majority) or lie in [1, %d], the number of files, not %d"
                         % (len(files), support))
    if area != -1 and area < 1:
        raise SystemExit("--consensus_area must be -1 (--domains_area's rule) or >= 1, not %d" % area)
    return files, None if support == -1 else support, None if area == -1 else area


def check_query(query, query_bed, query_bedpe, query_field, query_shift, resolution, segment, postprocess, compare, domains,
                render, tracks, enrich, pileup, consensus, ancestral, save_model, profile, filter_device, aggregate="", regrid=""):
    """--query FILE.mat with --query_bed FILE or --query_bedpe FILE reads one finished state map and a list of intervals: it
    goes with nothing that loads data or fits, and with no other reader of a state map -> the shift in bins, or None"""
    if not query:
        if query_bed or query_bedpe:
            raise SystemExit("--query_bed and --query_bedpe go with --query: the .mat to look the intervals up in")
        return None
    if bool(query_bed) == bool(query_bedpe):
        raise SystemExit("--query takes its intervals from --query_bed or from --query_bedpe: exactly one of the two")
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--compare", compare), ("--domains", domains),
                        ("--render", render), ("--tracks", tracks), ("--enrich", enrich), ("--pileup", pileup),
                        ("--consensus", consensus), ("--ancestral", ancestral), ("--save_model", save_model),
                        ("--profile 1", str(profile) == "1"), ("--filter_device 1", str(filter_device) == "1"),
                        ("--aggregate", aggregate), ("--regrid", regrid)):
        if value:
            raise SystemExit("--query cannot be combined with %s: it loads no data and fits nothing" % name)
    if query_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--query_field must be state_vec or state_vec_smooth, not %r" % (query_field,))
    from phylo_hmrf_amd.pileup import check_bins
    try:
        return check_bins(int(resolution), 0, int(query_shift))[1]
    except ValueError as e:
        raise SystemExit("--query with --query_shift %s: %s" % (query_shift, e))


def check_aggregate(aggregate, aggregate_bed, aggregate_bedpe, aggregate_field, aggregate_body, aggregate_flank, aggregate_shift,
                    aggregate_min, aggregate_colors, resolution, segment, postprocess, compare, domains, render, tracks, enrich,
                    pileup, consensus, query, ancestral, save_model, profile, filter_device, regrid=""):
    """--aggregate FILE.mat with --aggregate_bed FILE or --aggregate_bedpe FILE reads one finished state map and a list of
    features: it goes with nothing that loads data or fits, and with no other reader of a state map -> (the body, the flank
    in cells, the shift in bins, the shortest feature in bp), or None"""
    if not aggregate:
        if aggregate_bed or aggregate_bedpe:
            raise SystemExit("--aggregate_bed and --aggregate_bedpe go with --aggregate: the .mat to pile up")
        if (aggregate_field, str(aggregate_body), str(aggregate_flank), str(aggregate_shift), str(aggregate_min),
                aggregate_colors) != ("state_vec", "32", "16", "0", "0", ""):
            raise SystemExit("--aggregate_field, --aggregate_body, --aggregate_flank, --aggregate_shift, --aggregate_min and "
                             "--aggregate_colors go with --aggregate")
        return None
    if bool(aggregate_bed) == bool(aggregate_bedpe):
        raise SystemExit("--aggregate takes its features from --aggregate_bed or from --aggregate_bedpe: exactly one of the two")
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--compare", compare), ("--domains", domains),
                        ("--render", render), ("--tracks", tracks), ("--enrich", enrich), ("--pileup", pileup),
                        ("--consensus", consensus), ("--query", query), ("--ancestral", ancestral), ("--save_model", save_model),
                        ("--profile 1", str(profile) == "1"), ("--filter_device 1", str(filter_device) == "1"),
                        ("--regrid", regrid)):
        if value:
            raise SystemExit("--aggregate cannot be combined with %s: it loads no data and fits nothing" % name)
    if aggregate_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--aggregate_field must be state_vec or state_vec_smooth, not %r" % (aggregate_field,))
    from phylo_hmrf_amd.aggregate import MAX_BODY, MAX_FLANK
    from phylo_hmrf_amd.pileup import check_bins
    try:
        body, flank, min_bp = int(aggregate_body), int(aggregate_flank), int(aggregate_min)
    except ValueError:
        raise SystemExit("--aggregate_body, --aggregate_flank and --aggregate_min must be integers")
    if not 1 <= body <= MAX_BODY:
        raise SystemExit("--aggregate_body must lie in 1 .. %d cells, not %d" % (MAX_BODY, body))
    if not 0 <= flank <= MAX_FLANK:
        raise SystemExit("--aggregate_flank must lie in 0 .. %d cells, not %d" % (MAX_FLANK, flank))
    if min_bp < 0:
        raise SystemExit("--aggregate_min must be >= 0 bp, not %d" % min_bp)
    try:
        return body, flank, check_bins(int(resolution), 0, int(aggregate_shift))[1], min_bp
    except ValueError as e:
        raise SystemExit("--aggregate with --aggregate_shift %s: %s" % (aggregate_shift, e))


def check_regrid(regrid, regrid_from, regrid_like, regrid_field, regrid_cover, resolution, segment, postprocess, compare, domains,
                 render, tracks, enrich, pileup, consensus, query, aggregate, ancestral, save_model, profile, filter_device):
    """--regrid SRC.mat --regrid_from BP reads one finished state map and writes it on bins of --resolution bp: it goes with
    nothing that loads data or fits, and with no other reader of a state map -> (the source's bin size in bp, the cover in
    percent), or None.  Without --regrid a sub-option is told from its absence by its default text alone, as --aggregate's are:
    `--regrid_cover 50` and `--regrid_field state_vec` pass for no option, `--regrid_cover 50.0` is refused."""
    if not regrid:
        if (regrid_from, regrid_like, regrid_field, str(regrid_cover)) != ("", "", "state_vec", "50"):
            raise SystemExit("--regrid_from, --regrid_like, --regrid_field and --regrid_cover go with --regrid")
        return None
    if not regrid_from:
        raise SystemExit("--regrid needs --regrid_from: the bin size of the .mat in bp (--resolution is the target's)")
    for name, value in (("--segment", segment), ("--postprocess", postprocess), ("--compare", compare), ("--domains", domains),
                        ("--render", render), ("--tracks", tracks), ("--enrich", enrich), ("--pileup", pileup),
                        ("--consensus", consensus), ("--query", query), ("--aggregate", aggregate), ("--ancestral", ancestral),
                        ("--save_model", save_model), ("--profile 1", str(profile) == "1"),
                        ("--filter_device 1", str(filter_device) == "1")):
        if value:
            raise SystemExit("--regrid cannot be combined with %s: it loads no data and fits nothing" % name)
    if regrid_field not in ("state_vec", "state_vec_smooth"):
        raise SystemExit("--regrid_field must be state_vec or state_vec_smooth, not %r" % (regrid_field,))
    from fractions import Fraction
    from phylo_hmrf_amd.regrid import ratio
    try:
        src, cover = int(regrid_from), Fraction(str(regrid_cover))
    except (ValueError, ZeroDivisionError):
        raise SystemExit("--regrid_from must be an integer and --regrid_cover a number")
    if not 0 <= cover <= 100:
        raise SystemExit("--regrid_cover must lie in 0 .. 100 percent, not %s" % regrid_cover)
    try:
        ratio(src, int(resolution))
    except ValueError as e:
        raise SystemExit("--regrid with --regrid_from %s and --resolution %s: %s" % (regrid_from, resolution, e))
    return src, str(regrid_cover)


def run(num_states, chromvec, root_path, multiple, species_name, sort_states, run_id1, cons_param, method_mode,
        initial_mode, initial_weight, initial_weight1, initial_magnitude, position1, position2, filter_sigma, beta,
        beta1, num_neighbor, filter_mode, conv_threshold, estimate_type, simu_version, annotation, reload_mode,
        diagonal_type, m_iter, resolution, quantile, ref_species, output_path, synthetic="0", seed="", quiet="0",
        init_method="minibatch", warm_start="best", checkpoint="", checkpoint_every="1", resume="", energy_tol_ppb="10000",
        save_model="", segment="", postprocess="", smooth_window="5", smooth_area="-1", smooth_iter="1",
        filter_device="0", ancestral="", compare="", compare_with="", compare_field="state_vec", compare_match="0",
        compare_min_conf="0", compare_area="-1", profile="0", profile_quantiles="0.003,0.25,0.5,0.75,0.997",
        domains="", domains_field="state_vec", domains_area="-1", render="", render_field="state_vec", render_side="2048",
        render_colors="", render_outline="0", render_conf="0", render_mark="", tracks="", tracks_field="state_vec",
        tracks_dist="0-", enrich="", enrich_bed="", enrich_field="state_vec", enrich_dist="0-", enrich_segments="0",
        pileup="", pileup_bed="", pileup_bedpe="", pileup_field="state_vec", pileup_flank="1000000", pileup_shift="0",
        pileup_colors="", consensus="", consensus_field="state_vec", consensus_match="0", consensus_support="-1",
        consensus_area="-1", query="", query_bed="", query_bedpe="", query_field="state_vec", query_shift="0",
        enrich_null="0", enrich_null_min="1000000", enrich_null_seed="0", aggregate="", aggregate_bed="", aggregate_bedpe="",
        aggregate_field="state_vec", aggregate_body="32", aggregate_flank="16", aggregate_shift="0", aggregate_min="0",
        aggregate_colors="", regrid="", regrid_from="", regrid_like="", regrid_field="state_vec", regrid_cover="50"):
    resample = check_regrid(regrid, regrid_from, regrid_like, regrid_field, regrid_cover, resolution, segment, postprocess,
                            compare or compare_with, domains, render, tracks, enrich, pileup, consensus, query, aggregate,
                            ancestral, save_model, profile, filter_device)
    grid = check_aggregate(aggregate, aggregate_bed, aggregate_bedpe, aggregate_field, aggregate_body, aggregate_flank,
                           aggregate_shift, aggregate_min, aggregate_colors, resolution, segment, postprocess,
                           compare or compare_with, domains, render, tracks, enrich, pileup, consensus, query, ancestral,
                           save_model, profile, filter_device, regrid=regrid)
    check_query(query, query_bed, query_bedpe, query_field, query_shift, resolution, segment, postprocess,
                compare or compare_with, domains, render, tracks, enrich, pileup, consensus, ancestral, save_model, profile,
                filter_device, aggregate=aggregate, regrid=regrid)
    vote = check_consensus(consensus, consensus_field, consensus_match, consensus_support, consensus_area, segment, postprocess,
                           compare or compare_with, domains, render, tracks, enrich, pileup, ancestral, save_model, profile,
                           filter_device, query=query, aggregate=aggregate, regrid=regrid)
    check_pileup(pileup, pileup_bed, pileup_bedpe, pileup_field, pileup_flank, pileup_shift, resolution, segment, postprocess,
                 compare or compare_with, domains, render, tracks, enrich, ancestral, save_model, profile, filter_device,
                 consensus=consensus, query=query, aggregate=aggregate, regrid=regrid)
    check_enrich(enrich, enrich_bed, enrich_field, enrich_dist, enrich_segments, resolution, segment, postprocess,
                 compare or compare_with, domains, render, tracks, ancestral, save_model, profile, filter_device,
                 consensus=consensus, query=query, aggregate=aggregate, regrid=regrid)
    null = check_enrich_null(enrich, enrich_null, enrich_null_min, enrich_null_seed, resolution)
    check_tracks(tracks, tracks_field, tracks_dist, resolution, render, segment, postprocess, compare or compare_with, domains,
                 ancestral, save_model, profile, filter_device, consensus=consensus, query=query, aggregate=aggregate,
                 regrid=regrid)
    side = check_render(render, render_field, render_side, render_outline, render_conf, segment, postprocess,
                        compare or compare_with, domains, ancestral, save_model, profile, filter_device, consensus=consensus, query=query,
                        aggregate=aggregate, regrid=regrid)
    check_domains(domains, domains_field, segment, postprocess, compare or compare_with, ancestral, save_model, profile,
                  filter_device, consensus=consensus, query=query, aggregate=aggregate, regrid=regrid)
    profile_q = check_profile(profile, profile_quantiles, postprocess, compare, consensus=consensus, query=query, aggregate=aggregate,
                              regrid=regrid)
    check_compare(compare, compare_with, compare_field, compare_match, segment, postprocess, ancestral, save_model,
                  filter_device, consensus=consensus, query=query, aggregate=aggregate, regrid=regrid)
    check_ancestral(ancestral, segment, postprocess, regrid=regrid)
    filter_device = int(filter_device)
    if filter_device not in (0, 1):
        raise SystemExit("--filter_device must be 0 or 1")
    if filter_device and (int(reload_mode) == 1 or int(synthetic) > 0 or postprocess):
        raise SystemExit("--filter_device 1 runs the raw loader's filter on the GPU: it cannot be combined with --reload 1, "
                         "--synthetic or --postprocess, where nothing is filtered")
    if resample:
        from phylo_hmrf_amd.regrid import regrid_files
        out = regrid_files(regrid, str(output_path), resample[0], int(resolution), like=regrid_like, field=regrid_field,
                           cover=resample[1])
        print("regridded map written: %s" % out)
        return out
    if vote:
        from phylo_hmrf_amd.consensus import consensus_files
        files, support, area = vote
        out = consensus_files(files, str(output_path), int(resolution), field=consensus_field, match=bool(int(consensus_match)),
                              min_support=support, min_area=area)
        print("consensus written: %s" % out)
        return out
    if aggregate:
        from phylo_hmrf_amd.aggregate import aggregate_files
        out = aggregate_files(aggregate, str(output_path), int(resolution), field=aggregate_field, bed=aggregate_bed,
                              bedpe=aggregate_bedpe, body=grid[0], flank=grid[1], shift_bp=int(aggregate_shift), min_bp=grid[3],
                              palette_path=aggregate_colors)
        print("aggregate written: %s" % out)
        return out
    if query:
        from phylo_hmrf_amd.query import query_files
        out = query_files(query, str(output_path), int(resolution), field=query_field, bed=query_bed, bedpe=query_bedpe,
                          shift_bp=int(query_shift))
        print("query written: %s" % out)
        return out
    if pileup:
        from phylo_hmrf_amd.pileup import pileup_files
        out = pileup_files(pileup, str(output_path), int(resolution), field=pileup_field, bed=pileup_bed, bedpe=pileup_bedpe,
                           flank_bp=int(pileup_flank), shift_bp=int(pileup_shift), palette_path=pileup_colors)
        print("pile-up written: %s" % out)
        return out
    if enrich:
        from phylo_hmrf_amd.enrich import NullSizeError, enrich_files
        try:
            out = enrich_files(enrich, enrich_bed, str(output_path), int(resolution), field=enrich_field, window_bp=enrich_dist,
                               segments=str(enrich_segments) == "1", null=null[0], null_min_bp=int(enrich_null_min),
                               null_seed=null[2])
        except NullSizeError as e:
            raise SystemExit("--enrich_null: %s" % e)
        print("enrichment written: %s" % out)
        return out
    if tracks:
        from phylo_hmrf_amd.tracks import tracks_files
        out = tracks_files(tracks, str(output_path), int(resolution), field=tracks_field, windows_bp=tracks_dist)
        print("tracks written: %s" % out)
        return out
    if render:
        from phylo_hmrf_amd.render import render_files
        out = render_files(render, str(output_path), field=render_field, max_side=side, palette_path=render_colors,
                           outline=str(render_outline) == "1", use_conf=str(render_conf) == "1", mark_path=render_mark)
        print("images written: %s" % out)
        return out
    if domains:
        from phylo_hmrf_amd.domains import domains_files
        area = int(domains_area)
        out = domains_files(domains, str(output_path), int(resolution), field=domains_field,
                            min_area=None if area == -1 else area)
        print("domains written: %s" % out)
        return out
    if compare:
        from phylo_hmrf_amd.compare import compare_files
        area = int(compare_area)
        out = compare_files(compare, compare_with, str(output_path), int(resolution), field=compare_field,
                            match=bool(int(compare_match)), min_conf=float(compare_min_conf),
                            min_area=None if area == -1 else area)
        print("comparison written: %s" % out)
        return out
    if postprocess:
        from phylo_hmrf_amd.smooth import postprocess_file
        area = int(smooth_area)
        out = postprocess_file(postprocess, str(output_path), int(resolution), int(smooth_window),
                               None if area == -1 else area, int(smooth_iter))
        print("post-processing written: %s" % out)
        return out
    seg_model = None
    if segment:
        # the features must be made as the model's were: its settings win, an explicit different one is refused
        from phylo_hmrf_amd.model_io import load_model
        seg_model = load_model(segment)
        num_states, resolution, num_neighbor, filter_mode, filter_sigma, diagonal_type = segment_settings(
            seg_model, num_states, resolution, num_neighbor, filter_mode, filter_sigma, diagonal_type)
    run_id = int(run_id1)
    n_components1 = int(num_states)
    cons_param = float(cons_param)
    initial_mode = int(initial_mode)
    initial_weight, initial_weight1, initial_magnitude = float(initial_weight), float(initial_weight1), float(initial_magnitude)
    method_mode = int(method_mode)
    version = int(simu_version)
    beta, beta1 = float(beta), float(beta1)
    num_neighbor = int(num_neighbor)
    conv_threshold = float(conv_threshold)
    estimate_type = int(estimate_type)
    annotation = str(annotation)
    reload_mode = int(reload_mode)
    m_iter = int(m_iter)
    resolution = int(resolution)
    output_path = str(output_path)
    data_path = str(root_path)
    synthetic = int(synthetic)
    seed = None if seed == "" else int(seed)
    print("estimate type %d" % estimate_type)
    os.makedirs(output_path, exist_ok=True)
    rank, world = init_process_group()

    from phylo_hmrf_amd import mstep
    from phylo_hmrf_amd.tree import load_tree_files
    if seg_model is None and not mstep.native_available():      # (only the Python fall-back of the M-step uses worker processes: forked before the GPU is touched)
        mstep._pool(min(n_components1, os.cpu_count() or 1))

    start = time.time()
    x_max, species = float("nan"), None
    if synthetic > 0:
        from phylo_hmrf_amd import synthetic as _syn
        S = 4
        samples, len_vec, edge_list_vec, edge_list = synthetic_cache(synthetic, S, n_components1, num_neighbor, seed or 0)
        branch_list = [1.0] * (len(edge_list))
        write_cache(output_path, resolution, run_id, samples, edge_list_vec, len_vec)
    else:
        edge_list, branch_list, species = load_tree_files(data_path)       # phylo_hmrf.py:1607-1631
        if seg_model is not None and np.asarray(edge_list).reshape(-1, 2).tolist() != seg_model.edge_list.tolist():
            raise ValueError("the tree under --root_path is not the model's (--segment %s)" % segment)
        # (rank 0 looks, everybody follows: with --reload 1 no rank may find the cache half there while another writes it)
        have_cache = all_ranks_agree(all(os.path.exists(f) for f in cache_names(output_path, resolution, run_id)))
        if reload_mode == 1 and not have_cache:
            print("%s does not exist" % cache_names(output_path, resolution, run_id)[0])   # :1682-1684
            reload_mode = 0
        if reload_mode == 1:
            samples, len_vec, edge_list_vec = load_cache(output_path, resolution, run_id)
        else:
            from phylo_hmrf_amd import preprocess
            with open("%s/path_list.txt" % data_path) as f:                 # :1633-1639
                filename_list = [line.strip() for line in f if line.strip()]
            # path_list.txt holds the species' directories, relative to the working directory in the reference's example
            filename_list = [p if os.path.isabs(p) or os.path.isdir(p) else os.path.join(data_path, p) for p in filename_list]
            chrom_vec = list(range(1, 23)) if str(chromvec) == "-1" else [int(c) for c in str(chromvec).split(",")]
            ref_filename = "%s/%s.chrom.sizes" % (data_path, str(ref_species))
            quantile = int(quantile)
            qfile = "chrom_quantile_test.txt"                               # :1648-1664
            # (rank 0 looks, everybody follows -- as for the cache files: no rank may find the file half written by another;
            #  the file appears by rename, and x_max itself is rank 0's on every rank)
            if seg_model is not None and np.isfinite(seg_model.x_max):
                x_max = float(seg_model.x_max)                              # (the model's scale, not this data's)
            elif quantile == 0 and all_ranks_agree(os.path.exists(qfile)):
                x_max = float(np.median(np.atleast_2d(np.loadtxt(qfile, delimiter="\t"))[:, 6])) if rank == 0 else 0.0
            else:
                m_vec_list = preprocess.quantile_contact_vec(chrom_vec, resolution, ref_filename, filename_list, species)
                if rank == 0:
                    np.savetxt(qfile + ".tmp", m_vec_list, fmt="%.4f", delimiter="\t")
                    os.replace(qfile + ".tmp", qfile)
                x_max = float(np.median(m_vec_list[:, 6]))
            x_max = float(all_ranks_agree(x_max))
            print(x_max)
            samples, len_vec, edge_list_vec = preprocess.load_data_chromosome2(
                chrom_vec, x_max, 0, resolution, num_neighbor, int(filter_mode), float(filter_sigma), int(diagonal_type),
                ref_filename, filename_list, species, data_path, annotation, filter_device=bool(filter_device))
            write_cache(output_path, resolution, run_id, samples, edge_list_vec, len_vec)     # :1697-1704
    print("use time load data: %s" % (time.time() - start))
    print(samples.shape)
    print(np.asarray(len_vec))

    if method_mode == 1 and seg_model is not None:
        from phylo_hmrf_amd.hmrf import phyloHMRF
        model = phyloHMRF.from_model(seg_model, samples, len_vec, edge_list_vec, random_state=seed, quiet=bool(int(quiet)))
        print("segmenting...")
        start = time.time()
        res = model.segment()
        print("segment use time: %s %s" % (time.time() - start, res["timing"]))
        filename3 = "%s/segment_%d_%d.mat" % (output_path, run_id, n_components1)
        if rank == 0:
            scipy.io.savemat(filename3, {"state_vec": res["state_vec"], "len_vec": np.asarray(len_vec), "conf": res["conf"],
                                         "top": res["top"], "energy": res["energy"]})
        if ancestral:
            from phylo_hmrf_amd.ancestral import save_npz
            start = time.time()
            anc = model.ancestral(weighting=ancestral)
            print("ancestral use time: %s %s" % (time.time() - start, anc["timing"]))
            if rank == 0:
                leaves = species if species is not None else seg_model.species
                save_npz("%s/ancestral_%d_%d.npz" % (output_path, run_id, n_components1), anc, ancestral, len_vec, leaves)
        if profile_q is not None:
            write_profile(model, res["state_vec"], profile_q, output_path, run_id, n_components1,
                          species if species is not None else seg_model.species, rank)
        model.close()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return filename3
    if method_mode == 1:
        from phylo_hmrf_amd.hmrf import phyloHMRF
        # several GPUs: one process per GPU (init_process_group above); the blocks (and row tiles of the ones larger than a
        # GPU's share) are dealt to the ranks, every rank loads the data, rank 0 writes the result
        tree1 = phyloHMRF(n_components=n_components1, run_id=run_id, n_samples=samples.shape[0],
                          n_features=samples[0].shape[-1], observation=samples, edge_list=edge_list, len_vec=len_vec,
                          type_id=version, branch_list=branch_list, edge_list_1=edge_list_vec, cons_param=cons_param,
                          beta=beta, beta1=beta1, initial_mode=initial_mode, initial_weight=initial_weight,
                          initial_weight1=initial_weight1, initial_magnitude=initial_magnitude, learning_rate=0.001,
                          estimate_type=estimate_type, max_iter=100, n_iter=5000, tol=1e-7, num_neighbor=num_neighbor,
                          random_state=seed, quiet=bool(int(quiet)), init_method=init_method, warm_start=warm_start,
                          checkpoint_path=checkpoint or None, checkpoint_every=int(checkpoint_every), resume_from=resume or None,
                          solver_opts=dict(energy_tol_ppb=int(energy_tol_ppb)))
        print("fitting...")
        lambda_0 = cons_param
        filename = "%s/estimate_ou_%d_%.2f_%d_%s" % (output_path, run_id, lambda_0, n_components1, annotation)
        start = time.time()
        params_vec1, params_vec2, params_vecList, iter_id1, iter_id2, cost_vec, state_vec = tree1.fit_accumulate_test(
            samples, len_vec, conv_threshold, filename, m_iter)
        print("fit use time: %s" % (time.time() - start))
        mdict = {"state_vec": state_vec, "len_vec": np.asarray(len_vec), "params_vec1": params_vec1,
                 "params_vec2": params_vec2, "iter_id1": iter_id1, "iter_id2": iter_id2, "cost_vec": cost_vec}
        filename3 = "%s/estimate_ou_%d_%.2f_%d.mat" % (output_path, run_id, lambda_0, n_components1)
        if rank == 0:                                   # (every rank holds the same result: state_vec is all-reduced)
            scipy.io.savemat(filename3, mdict)
        if save_model and rank == 0:
            pre = {} if synthetic > 0 else dict(x_max=x_max, resolution=resolution, filter_mode=int(filter_mode),
                                                 filter_sigma=float(filter_sigma), diagonal_type=int(diagonal_type))
            tree1.save_model(save_model, species=species, **pre)
        if profile_q is not None:
            write_profile(tree1, state_vec, profile_q, output_path, run_id, n_components1, species, rank)
        print(params_vecList.shape)
        tree1.close()
        mstep.close_pool()
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
        return filename3
    mstep.close_pool()
    return None


if __name__ == "__main__":
    opts = parse_args()
    run(opts.num_states, opts.chromvec, opts.root_path, opts.multiple, opts.species_name, opts.sort_states, opts.run_id,
        opts.cons_param, opts.method_mode, opts.initial_mode, opts.initial_weight, opts.initial_weight1,
        opts.initial_magnitude, opts.position1, opts.position2, opts.filter_sigma, opts.beta, opts.beta1,
        opts.num_neighbor, opts.filter_mode, opts.threshold, opts.estimate_type, opts.simu_version, opts.annotation,
        opts.reload, opts.dtype, opts.miter, opts.resolution, opts.quantile, opts.ref_species, opts.output,
        synthetic=opts.synthetic, seed=opts.seed, quiet=opts.quiet, init_method=opts.init, warm_start=opts.warm_start,
        checkpoint=opts.checkpoint, checkpoint_every=opts.checkpoint_every, resume=opts.resume,
        energy_tol_ppb=opts.energy_tol_ppb, save_model=opts.save_model, segment=opts.segment,
        postprocess=opts.postprocess, smooth_window=opts.smooth_window, smooth_area=opts.smooth_area,
        smooth_iter=opts.smooth_iter, filter_device=opts.filter_device, ancestral=opts.ancestral,
        compare=opts.compare, compare_with=opts.compare_with, compare_field=opts.compare_field,
        compare_match=opts.compare_match, compare_min_conf=opts.compare_min_conf, compare_area=opts.compare_area,
        profile=opts.profile, profile_quantiles=opts.profile_quantiles, domains=opts.domains,
        domains_field=opts.domains_field, domains_area=opts.domains_area, render=opts.render,
        render_field=opts.render_field, render_side=opts.render_side, render_colors=opts.render_colors,
        render_outline=opts.render_outline, render_conf=opts.render_conf, render_mark=opts.render_mark,
        tracks=opts.tracks, tracks_field=opts.tracks_field, tracks_dist=opts.tracks_dist, enrich=opts.enrich,
        enrich_bed=opts.enrich_bed, enrich_field=opts.enrich_field, enrich_dist=opts.enrich_dist,
        enrich_segments=opts.enrich_segments, pileup=opts.pileup, pileup_bed=opts.pileup_bed, pileup_bedpe=opts.pileup_bedpe,
        pileup_field=opts.pileup_field, pileup_flank=opts.pileup_flank, pileup_shift=opts.pileup_shift,
        pileup_colors=opts.pileup_colors, consensus=opts.consensus, consensus_field=opts.consensus_field,
        consensus_match=opts.consensus_match, consensus_support=opts.consensus_support, consensus_area=opts.consensus_area,
        query=opts.query, query_bed=opts.query_bed, query_bedpe=opts.query_bedpe, query_field=opts.query_field,
        query_shift=opts.query_shift, enrich_null=opts.enrich_null, enrich_null_min=opts.enrich_null_min,
        enrich_null_seed=opts.enrich_null_seed, aggregate=opts.aggregate, aggregate_bed=opts.aggregate_bed,
        aggregate_bedpe=opts.aggregate_bedpe, aggregate_field=opts.aggregate_field, aggregate_body=opts.aggregate_body,
        aggregate_flank=opts.aggregate_flank, aggregate_shift=opts.aggregate_shift, aggregate_min=opts.aggregate_min,
        aggregate_colors=opts.aggregate_colors, regrid=opts.regrid, regrid_from=opts.regrid_from, regrid_like=opts.regrid_like,
        regrid_field=opts.regrid_field, regrid_cover=opts.regrid_cover)
