"""Command line of the MI355X path, keeping the flag names and defaults of /root/reference/chexpert.py:29-57
(`--train`, `--evaluate_single_model`, `--evaluate_ensemble`, `--visualize`, `--plot_roc`, `--model`, `--batch_size 16`,
`--lr 1e-4`, `--n_epochs 1`, `--log_interval 50`, `--eval_interval 300`, `--lr_decay_factor 0.97`, `--lr_warmup_steps`,
`--resize`, `--mini_data`, `--cuda`, `--restore`, `--load_config`, `--seed`), plus

  --evaluate            alias of --evaluate_single_model (BASELINE.json spells it that way)
  --synthetic N         N hash-generated uint8 X-rays with U-Ones-like labels (the CheXpert images are not available offline)
  --n_classes K         5 = the reference's competition labels (chexpert.py:460)
  --dtype {bf16,fp32}   activation storage of the fused schedule (fp32 = the 1e-3 parity mode, densenet121)
  --fused_optimizer     one-kernel optimiser on the flat parameter buffer; with --graph the whole step (forward, loss, backward,
                        optimiser, scheduler) is captured once as a hipGraph and replayed per minibatch
  --jitter              brightness / contrast jitter +-0.25 of the uint8 image on the GPU (the reference's `_data_aug` rows)
  --affine              random rotation / translation / scale / shear of the uint8 image on the GPU (training only; it runs before
                        --jitter: geometric first, photometric second), ranges as torchvision's RandomAffine:
                        --affine_degrees 10, --affine_translate 0.05, --affine_scale 0.9 1.1, --affine_shear 0
  --clahe               contrast-limited adaptive histogram equalisation of the uint8 image on the GPU (chexpert_amd/augment.py):
                        deterministic preprocessing, so it runs in EVERY mode (training, its evaluations, --evaluate_single_model,
                        --evaluate_ensemble, --visualize), as the first step on the uint8 batch, before --affine and --jitter;
                        --clahe_grid 8 8 tiles (each 1..16, dividing the crop size), --clahe_clip 2.0 (0: no clipping).  It sits behind
                        the loader: --cache_decoded does not depend on these settings
  --mixup ALPHA         sample-mixing regularisation of the uint8 batch and its targets on the GPU (chexpert_amd/augment.py: SampleMix;
  --cutmix ALPHA        training only), the LAST step on the batch, after --clahe, --affine and --jitter (per-sample transforms first,
                        then the collated batch is mixed, as timm does): Mixup blends every image with a partner of the minibatch at
                        lambda ~ Beta(ALPHA, ALPHA), CutMix pastes a box of the partner (area share 1 - lambda); the targets are blended
                        by the same share, a label the loss ignores (-1) stays ignored.  0 (default): off.  With both, CutMix is chosen
                        with --mix_switch_prob P (default 0.5); --mix_prob P: the probability that a minibatch is mixed at all (default
                        1.0); --mix_mode batch|elem: one draw per minibatch (default) or per image.  Not with --loss aucm (it thresholds
                        the targets at 0.5).  Each data-parallel rank mixes its own shard with its own seed
  --erase_prob P        random erasing (Cutout) of the uint8 batch on the GPU, after the mix: each image with probability P gets one
                        rectangle (area 2 % .. 1/3 of the image, aspect 0.3 .. 3.3, as torchvision's RandomErasing) overwritten with the
                        grey level --erase_fill V (default 136, the dataset mean); labels do not change.  0 (default): off
  --uncertain POLICY    what an uncertain (-1) training label becomes: ones (the reference's U-Ones, default), zeros, ignore (it stays
                        -1 and the loss skips it), ones_lsr / zeros_lsr (label smoothing: uniform in [0.55, 0.85] / [0, 0.3]),
                        multiclass (the paper's U-MultiClass: it stays -1 and is a class of its own).  multiclass is a different
                        model, not a different table: every model family gets a head of 3 x n_classes outputs (negative, positive,
                        uncertain per finding; --n_classes stays the number of findings) and trains a three-way softmax cross-entropy
                        per finding, inside the fused step (FusedNet.set_loss(kind="multiclass"), cx_mc3_fwd_bwd) and, without
                        --fused_optimizer, through loss.MultiClassUncertain.  Evaluation drops the uncertain output right after the
                        forward (loss.collapse_multiclass: z = z_positive - z_negative, sigmoid(z) = p1 / (p0 + p1)), so the evaluation
                        loss (cross-entropy on z), AUROC, --bootstrap*, --calibrate*, --plot_roc, --evaluate_ensemble and the
                        eval_results files see (N, n_classes) logits as always.  The checkpoint carries `loss_state`; --restore
                        refuses a checkpoint of the other head, both ways (evaluating a multiclass checkpoint needs the flag too).
                        Works with --fused_optimizer --graph, --erase_prob and more than one rank.  Not with --loss other than bce,
                        --pos_weight, --mixup / --cutmix (no soft-target form) or --visualize (the class indices of the CAM and
                        saliency tools are head outputs)
  --pos_weight W        `auto` or n_classes floats: BCEWithLogitsLoss's pos_weight, inside the fused step too; auto = per class
                        (non-ignored negatives) / (positives) of the training labels, clamped to [1/16, 16]
  --loss {bce,aucm}     aucm: the AUC min-max-margin loss (Yuan et al., ICCV 2021; FusedNet.set_loss(kind="aucm"), loss.AUCMLoss) instead of
                        the cross-entropy, its auxiliary scalars trained beside the network: --aucm_margin M (default 1.0), --aucm_prior `auto`
                        (the default) or n_classes positive rates in (0, 1); auto = per class positives / non-ignored labels of the
                        training table, a label >= 0.5 being a positive; --aucm_lr_aux R, the rate of the auxiliary scalars (default:
                        --lr).  Not with --pos_weight, and on one GPU only.  Evaluation keeps reporting cross-entropy element losses
  --loss {focal,asl}    the focal loss (Lin et al., ICCV 2017) / the asymmetric loss (Ridnik et al., ICCV 2021) instead of the cross-entropy,
                        inside the fused step (FusedNet.set_loss(kind="focal" | "asl"), cx_asl_fwd_bwd) and, without --fused_optimizer,
                        through loss.FocalLoss / loss.AsymmetricLoss: --focal_gamma G (default 2), --focal_alpha A (in (0, 1); default
                        none); --asl_gamma_pos GP (default 0), --asl_gamma_neg GN (default 4), --asl_clip M (in [0, 1); default 0.05).
                        Both skip an ignored (-1) label and take soft labels, so they combine with --uncertain, --pos_weight (also
                        auto), --mixup / --cutmix / --erase_prob, --fused_optimizer --graph and more than one rank.  The evaluation
                        loss in eval_results stays the (masked) cross-entropy, so it can be compared across training losses; the
                        checkpoint carries the loss's four numbers (`loss_state`), which --restore puts back
  --labels {competition,all}
                        the findings read from the csv: the five competition labels (default) or all 14, in the csv's column order
                        (data.ATTR_NAMES_ALL); all sets --n_classes 14 and refuses another one
  --loss hier           the hierarchical label loss over the findings' tree (Chen et al., MIDL 2019; Pham et al., 2019), inside the fused
                        step (FusedNet.set_loss(kind="hier"), cx_hier_fwd_bwd) and, without --fused_optimizer, through
                        loss.HierarchicalBCE: every logit is that of P(finding | its parent is positive).  --hier_mode conditional
                        (default: the masked cross-entropy where every ancestor's label is positive) or unconditional (the
                        cross-entropy of the product of probabilities along the path); --hier_parents `auto` (default: the CheXpert
                        tree data.CHEXPERT_PARENT, needs --labels all) or n_classes integers, each label's parent or -1, parents first
                        (synthetic data, other label sets).  The label tables get data.hierarchy_closure after the --uncertain policy
                        (a positive child makes its ancestors positive; --no_hier_closure leaves them).  Evaluation turns the
                        conditional logits into unconditional ones right after the forward (loss.collapse_hierarchy), so the
                        evaluation loss, AUROC, --bootstrap*, --delong, --calibrate*, --plot_roc, --evaluate_ensemble and the
                        eval_results files see them; the maps of --visualize are those of the conditional logits.  The checkpoint
                        carries kind, table, mode and the closure choice (`loss_state`); --restore and --evaluate_* read them: a run
                        without --hier_mode continues in the stored mode, a --hier_parents or --hier_mode that contradicts them
                        is refused, and an evaluation without --loss hier closes its validation table iff the training run did
                        (with --loss hier the run's own --no_hier_closure decides).  Takes --pos_weight, --uncertain (but multiclass), --fused_optimizer --graph and more
                        than one rank; not with --mixup / --cutmix, nor with the five competition labels and `auto`
  --pool KIND           the global pooling in front of the classifier (FusedNet.set_pool, csrc/pool_head.hip): avg (default), max, lse
                        (log-sum-exp, --pool_r R: sharpness, default 10) or gem (generalised mean, --pool_p P: start of the trained
                        exponent in [1, 16], default 3); every --model, with --fused_optimizer --graph and more than one rank.  The
                        checkpoint of another pooling than the average carries `pool_state`; --restore, --evaluate_*, --visualize and predict.py read the kind from it, a
                        --pool that names another kind is refused.  Grad-CAM and --cam_classes assume the average: --visualize on
                        another pooling draws the --saliency figures only
  --head KIND           the head of the network (FusedNet.set_head, csrc/csra_head.hip): linear (default: activation, pool, classifier) or
                        csra, class-specific residual attention: the classifier at every pixel, the score map pooled per class by its
                        mean plus --csra_lambda L (default 0.1) times its softmax-weighted mean at temperature --csra_T T (default 1);
                        every --model, with --fused_optimizer --graph and more than one rank; it stands on the average pool (not
                        with --pool max / lse / gem).  The checkpoint of a csra run carries `head_state`; --restore, --evaluate_*,
                        --visualize and predict.py read the head from it, and --head linear is then refused.  A checkpoint of a
                        linear-head run may be restored into --head csra (the keys are equal: fine-tuning).  --visualize
                        --cam_classes on a csra model writes vis/csra_maps_lowres.npy (N, 2, K, h, w): the scores and the attention
                        of the requested classes (heads.class_maps).
                        pcam is probabilistic-CAM pooling (Ye et al. 2020): the classifier at every pixel, each per-pixel logit turned
                        into a probability, the map pooled per class with those probabilities as weights; no hyper-parameter
                        (--csra_lambda / --csra_T are refused), the average pool only, checkpoints and --restore as for csra.  A
                        linear-head checkpoint may be restored into --head pcam (the keys are equal), but the function changes, unlike
                        csra at lambda 0.  --visualize --cam_classes on a pcam model writes vis/pcam_maps_lowres.npy (N, 2, K, h, w),
                        the probability maps P in [0, 1] and the pooling weights, and one vis/pcam_<ident>_step_<N>.png per image
  --cam_classes [C ...] with --visualize: class-specific maps (gradcam.class_cam) of the 'vis' subset for these class indices (no value
                        or `all`: every class): vis/class_cam_lowres.npy (N, K, h, w) and one vis/classcam_<ident>_step_<N>.png per image
  --saliency METHOD     with --visualize: full-resolution, class-specific pixel attributions (chexpert_amd/saliency.py) of the 'vis' subset:
                        grad (|d logit / d x|), smoothgrad, smoothgrad_sq or ig (integrated gradients, signed).  --saliency_classes
                        [C ...] (as --cam_classes; default all), --saliency_steps M (path steps of ig, default 32; noise samples of
                        smoothgrad, default 16), --saliency_sigma S (noise in whitened units; default 0.15 of the uint8 range),
                        --saliency_baseline mean|black (ig; default mean), --saliency_chunk R (rows per pass).  Writes
                        vis/saliency_<method>.npy (N, K, H, W) fp16, every map divided by its largest magnitude, those magnitudes in
                        vis/saliency_<method>_scale.npy (N, K) fp32, and one vis/saliency_<method>_<ident>_step_<N>.png per image
  --synthetic_uncertain F   that fraction of the synthetic training labels is uncertain (the policy above then applies)
  --clip_grad_norm X    clip the gradient to global L2 norm X inside the fused optimiser step (needs --fused_optimizer, as the next three)
  --skip_nonfinite      drop the update of a minibatch whose gradient norm is inf or NaN (it still counts for the schedule)
  --ema_decay D         exponential moving average of the weights, written by the optimiser kernel; evaluation and the checkpoint's
                        `ema_state_dict` use it.  --no_ema_warmup: constant decay instead of min(D, (1 + step) / (10 + step))
  --use_ema             --evaluate_single_model / --evaluate_ensemble / --visualize load `ema_state_dict` from the checkpoint
  --weight_decay W      weight decay of the fused optimiser (needs --fused_optimizer, as the next five); L2 (g += W p) unless
                        --decoupled_decay: p <- p (1 - lr W) ahead of the update (AdamW's rule, for all three optimisers)
  --no_decay_norm_bias  no weight decay on 1-D parameters (BatchNorm weights and biases, every bias)
  --head_lr_mult M / --backbone_lr_mult M   learning-rate multiplier of the classifier (the last nn.Linear) / of everything else
  --freeze_backbone_steps N   the classifier trains alone for the first N minibatches, then the backbone is thawed (-1: for the whole
                        run, a linear probe).  The backward pass still fills every gradient and BatchNorm running statistics keep
                        moving; the optimiser kernels skip the frozen tensors.  Works with --graph (the group table lives on the device)
  --optimizer lamb|lars the layer-wise trust-ratio optimisers (optim.FusedLAMB on Adam, optim.FusedLARS on SGD with Nesterov momentum and its
                        MultiStepLR) instead of the model's own, for every --model (needs --fused_optimizer): each tensor's update is
                        rescaled by |p| / |update|, computed inside the step on the device, so one --lr serves every layer at a large
                        global batch.  Works with --graph, more than one rank, --clip_grad_norm, --skip_nonfinite, --ema_decay,
                        --weight_decay, --no_decay_norm_bias (the 1-D parameters then get neither decay nor adaptation),
                        --head_lr_mult, --backbone_lr_mult and --freeze_backbone_steps; not with --decoupled_decay (LAMB's decay
                        already sits outside the moments, LARS's is part of the ratio).  --trust_coef C: the coefficient of lars
                        (default 0.001; lars only); --trust_clip: ratios capped at 1; --always_adapt: tensors without weight decay are
                        adapted too.  The json log line gains trust_min / trust_max over the adapted tensors.  --restore of a
                        checkpoint written under another optimiser is refused
  --sam_rho R           R > 0: sharpness-aware minimisation (optim.FusedSAM) around the fused optimiser the other flags choose (needs
                        --fused_optimizer): each step takes the gradient twice, the second time at the weights moved by R along the
                        normalised first gradient, which costs a second forward/backward pass; --sam_adaptive: the scale-invariant
                        form (ASAM: the step is scaled by the weights, elementwise).  Works with and without --graph, every
                        --optimizer, --loss (but aucm), --pool and --head and the clip / skip / EMA / group flags; not on more than
                        one rank.  The json log line gains sam_norm; the optimiser checkpoint carries a `sam` entry beside the
                        base optimiser's state, so --restore of a SAM run into a run without it, and the reverse, both work
  --bootstrap B         B > 0: every eval_results_<tag>.json gets an auc_ci_<tag>.json beside it (rank 0): AUROC per class and for the mean
                        with its (1 - A) percentile bootstrap interval over B replicates, computed on the GPU (metrics.bootstrap_auc);
                        --bootstrap_seed S (default: --seed), --bootstrap_unit image|study|patient (what is resampled; study and
                        patient need the real data's paths), --bootstrap_alpha A (default 0.05).  0 (default): nothing is computed,
                        allocated or written
  --bootstrap_metrics M [M ...]   with --bootstrap B > 0: a metrics_ci_<tag>.json beside every auc_ci_<tag>.json, with the same seed, unit and
                        level: the interval of every named metric over the same kind of resamples (metrics.bootstrap_metrics): auroc, ap
                        (average precision), sens@S (sensitivity at specificity >= S), spec@S (specificity at sensitivity >= S), S inside
                        (0, 1) with at most 6 decimals, at most 8 operating points.  Not given (default): nothing more is computed or written
  --delong              every eval_results_<tag>.json gets a delong_<tag>.json beside it (rank 0): AUROC per class and for the mean with its
                        analytic standard error and (1 - A) normal interval, computed on the GPU (metrics.delong_auc): DeLong's variance
                        for --bootstrap_unit image, Obuchowski's clustered extension for study / patient (which need the real data's
                        paths); A is --bootstrap_alpha.  Deterministic, no replicates.  With --evaluate_ensemble, delong_ensemble.json
                        also holds under "vs_members" DeLong's paired test of the ensemble against every member checkpoint
                        (metrics.delong_auc_diff).  Not given (default): nothing is computed, allocated or written
  --calibrate temperature|platt   every eval_results_<tag>.json gets a calibration_<tag>.json beside it (rank 0): the per-class map
                        p = sigmoid(a z + b) fitted on the GPU on that evaluation's logits (temperature: b = 0), ECE / MCE / Brier score
                        before and after it, the reliability curves and, with --bootstrap B, the intervals of all six (same seed, unit
                        and level as the AUROC intervals; conditional on the fit), plus reliability_<tag>.png.  --calibrate_smooth: Platt's
                        smoothed targets (the cure for a separable class); --calibration_bins M (1 .. 64, default 15),
                        --calibration_binning width|mass (equal-width bins of [0, 1) or equal-mass bins of the scores)
  --calibration_from FILE   apply the fit stored in FILE (a calibration_<tag>.json, e.g. of another split) instead of fitting; exclusive with
                        --calibrate.  Before / after measured on the split the map was fitted on is optimistic: fit on one split, report
                        on another.  --calibration_bins alone applies no map and reports the uncalibrated metrics only
  --pretrain contrastive   contrastive pretraining of the backbone on the images themselves (SimCLR's NT-Xent, SupCon's L_out with several
                        positives; MoCo-CXR and MedAug are the sources for chest X-rays): the classifier nn.Linear becomes the projection of
                        width --proj_dim D (default 128), every minibatch is equalised once (--clahe), duplicated into [x; x] and each copy
                        gets its own --affine / --jitter draw, and the step's loss is FusedNet.set_loss(kind="ntxent", temperature=T)
                        with --temperature T (default 0.2) over the 2 x --batch_size rows (both views share BatchNorm's batch
                        statistics).  --positive view (default): the two views of an image are each other's only positives; study |
                        patient: every row of the same study / patient in the minibatch is one (MedAug; needs the real data's paths).  The
                        labels are not read.  Needs --train and --affine or --jitter; refuses --mixup / --cutmix / --erase_prob, --loss,
                        --pos_weight, --uncertain multiclass, --head csra|pcam, more than one rank and the --evaluate_* / --visualize /
                        --plot_roc modes.  An --eval_interval step computes the contrastive loss and the top-1 share (the anchors whose
                        nearest row is a positive) over the validation set from two views drawn from a fixed seed, prints them and writes
                        pretrain_eval_step_<n>.json; the checkpoint carries loss_state, "pretrain": "contrastive" and eval_loss, and its
                        avg_auc is -eval_loss, so that the best_checkpoints are the lowest-loss ones.  --restore continues such a run and
                        is refused into a supervised one (and the other way round); the log line gains top1
  --pretrain barlow     Barlow Twins pretraining (Zbontar et al., ICML 2021), the pretext loss that needs neither negatives nor a large
                        batch: the same two views as --pretrain contrastive (needs --train and --affine or --jitter, refuses what it
                        refuses), but the step's loss is FusedNet.set_loss(kind="barlow", lambd=L) with --barlow_lambda L (default 0.0051,
                        the paper's): both views' embeddings are batch-normalised over the minibatch and their cross-correlation matrix is
                        pushed towards the identity (csrc/barlow.hip, on the fp32-input MFMA).  --proj_dim D defaults to 512 here (1 ..
                        1024); --temperature and --positive study|patient are refused.  The log line gains on_diag / off_diag; an
                        evaluation writes pretrain_eval_step_<n>.json with "pretrain": "barlow", "loss": {"barlow": the mean over the
                        validation minibatches weighted by their pairs}, on_diag, off_diag, mean_diag, pairs and lambda (and the
                        --knn_probe / --linear_probe results); the checkpoint carries "pretrain": "barlow"; --restore continues such a run
                        (the stored lambda is used unless --barlow_lambda is given) and is refused into a supervised or a contrastive one,
                        --init_backbone takes its backbone as it takes a contrastive checkpoint's
  --knn_probe K         the weighted k-nearest-neighbour probe of the backbone (Wu et al., CVPR 2018; chexpert_amd/knn.py, csrc/knn.hip): a bank
                        of training images and the validation set are embedded with the frozen network in eval mode (FusedNet.embed: the
                        pooled features the classifier reads; the deterministic preprocessing only, --clahe if set, no views), each
                        validation image's K nearest bank rows by cosine similarity (1 <= K <= 256, cut to the bank's size) vote on its
                        findings with weight exp(s / T), --knn_temperature T (default 0.1), and the AUROC per finding is reported.
                        --knn_bank N (default 8192): the bank is N training images at an even stride, the same ones every time; 0 = the
                        whole training set.  The bank's labels follow --uncertain / --labels, an ignored (-1) label does not vote.  With
                        --pretrain contrastive every evaluation adds "knn": {k, temperature, bank, aucs, mean_auc} to
                        pretrain_eval_step_<n>.json and prints one line (checkpoint selection stays by the contrastive loss); with
                        --evaluate_single_model it writes knn_step_<n>.json beside eval_results_step_<n>.json, for any checkpoint.
                        Needs one of the two modes, one rank and the linear head (not --head csra|pcam)
  --linear_probe        the linear evaluation of the backbone (SimCLR, MoCo, MoCo-CXR; chexpert_amd/probe.py, csrc/probe.hip): the bank and
                        the validation set are embedded as for --knn_probe (once where both are given and read the same bank), then one
                        logistic regression per finding is fitted on the bank's standardised features by L-BFGS on the GPU -- no backward
                        pass through the network, and the result is the optimum, the same for the same checkpoint -- and the AUROC per
                        finding on the validation set is reported.  --probe_l2 L [L ...] (default 0.001): one fit per value, in descending
                        order, each warm-started from the one before; the report lists every value, the choice is the reader's.
                        --probe_bank N (default 8192; 0 = the whole training set) at an even stride: a label fraction.  The labels are the
                        training table's (--uncertain / --labels); an ignored (-1) label is no row of its finding.  --probe_max_iter I
                        (default 200).  With --pretrain contrastive every evaluation adds "linear_probe": {bank, l2, fits: [{l2, aucs,
                        mean_auc, status, iterations, passes, train_loss}]} to pretrain_eval_step_<n>.json and prints one line; with
                        --evaluate_single_model it writes probe_step_<n>.json beside eval_results_step_<n>.json.  --probe_save FILE
                        (--evaluate_single_model and exactly one --probe_l2): a checkpoint of the restored weights with the classifier
                        replaced by the fit (folded back to raw features), the pooling's numbers kept, no optimiser and no loss state
                        (the probe is a BCE model), the step the source's: --restore FILE --evaluate_single_model evaluates it.  Needs
                        one of the two modes, one rank, the linear head and one logit per finding (not --uncertain multiclass, --loss hier)
  --init_backbone FILE  with --train: every tensor of FILE's state_dict but the classifier's weight and bias (whatever their width) is loaded
                        before the first step, BatchNorm's running statistics included (the pooling's own numbers, GeM's exponent and
                        log-sum-exp's sharpness, where the checkpoint and this run's --pool both have them); the step, the
                        optimiser state and the loss state are not.  A missing or mis-shaped key is an error that names it.  --pool, --head
                        and --loss stay free; exclusive with --restore.  (The linear evaluation of such a backbone is --linear_probe)

Data parallel: launch with `python -m torch.distributed.run --nproc-per-node N chexpert.py --train ...`; every rank holds a
replica and a shard of each minibatch stream (per-rank BatchNorm statistics, averaged gradients: DDP semantics), the
validation set is sharded too and its logits are gathered to rank 0, which alone writes checkpoints and results.
Images travel as decoded grey bytes (1 B per pixel); whitening `(u/255 - 0.5330)/0.0349` and the expansion to three identical
channels (chexpert.py:70-72) happen on the GPU.  Logging goes to stdout / JSON (tensorboardX is not used).

`main()` is a sequence of phases, each a function of this module; what a later phase reads of an earlier one travels in one
plain container (`run`, a SimpleNamespace without methods):

  1. check_flags               every refusal a flag earns on its own, before a process group, a directory or a dataset exists
  2. open_output_dir           --output_dir and config.json (add_to_config: a resolved key of a config this run created)
  3. load_datasets             synthetic or ChexpertCSV, the decoded cache, the hierarchy closure; resolve_label_statistics
  4. make_loader               the RingLoader, before the first GPU call; from here to the end of training one try/finally closes it
  5. build_model               restore_source / restore_pool / restore_head / make_model / restore / hier_for_checkpoint / init_backbone
  6. wire_loss                 FusedNet.set_loss, the autograd route's criterion, the AUCM module and its optimiser
  7. train                     the epoch loop: preprocess, then the graphed / eager / autograd step, log_line, evaluate_and_checkpoint;
                               every fused step is `optimizer.train_step(model, x, t, dev=...)` (optim._Flat, optim.FusedSAM), replayed
                               from graph.GraphedTrainStep / SegmentedTrainStep or launched one by one
  8. run_eval / evaluate_ensemble / visualize / plot_all_roc, and the process group's teardown
"""
import argparse
import contextlib
import json
import os
import pprint
import time
import types

import numpy as np
import torch
import torch.nn as nn

from . import metrics as M
from . import parallel as P
from . import synth
from .data import UNCERTAIN_POLICIES, apply_uncertain

BOOTSTRAP_UNITS = ("image", "study", "patient")
ATTR_NAMES = ["Atelectasis", "Cardiomegaly", "Consolidation", "Edema", "Pleural Effusion"]     # dataset.py:25


def build_parser():
    p = argparse.ArgumentParser(description="CheXpert classifiers on MI355X (HIP kernels)")
    p.add_argument("--load_config", type=str)
    p.add_argument("--train", action="store_true")
    p.add_argument("--evaluate_single_model", "--evaluate", dest="evaluate_single_model", action="store_true")
    p.add_argument("--evaluate_ensemble", action="store_true")
    p.add_argument("--visualize", action="store_true")
    p.add_argument("--plot_roc", action="store_true")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--cuda", type=int, default=0)
    p.add_argument("--data_path", default="")
    p.add_argument("--output_dir")
    p.add_argument("--restore", type=str)
    p.add_argument("--model", default="densenet121")
    p.add_argument("--mini_data", type=int)
    p.add_argument("--resize", type=int)
    p.add_argument("--pretrained", action="store_true")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--n_epochs", type=int, default=1)
    p.add_argument("--lr", type=float, default=1e-4)
    p.add_argument("--lr_warmup_steps", type=float, default=0)
    p.add_argument("--lr_decay_factor", type=float, default=0.97)
    p.add_argument("--step", type=int, default=0)
    p.add_argument("--log_interval", type=int, default=50)
    p.add_argument("--eval_interval", type=int, default=300)
    p.add_argument("--synthetic", type=int, default=0, help="number of synthetic training images (no dataset offline)")
    p.add_argument("--n_classes", type=int, default=len(ATTR_NAMES))
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--fused_optimizer", action="store_true", help="one-kernel optimiser on the flat parameter buffer")
    p.add_argument("--graph", action="store_true", help="capture the training step as a hipGraph (needs --fused_optimizer)")
    p.add_argument("--jitter", action="store_true", help="brightness / contrast jitter +-0.25 on the uint8 image (GPU)")
    p.add_argument("--affine", action="store_true", help="random affine warp of the uint8 image (GPU, training only)")
    p.add_argument("--affine_degrees", type=float, default=10.0, help="rotation uniform in +-degrees")
    p.add_argument("--affine_translate", type=float, default=0.05, help="translation uniform in +-fraction of the image size, per axis")
    p.add_argument("--affine_scale", type=float, nargs=2, default=[0.9, 1.1], metavar=("LO", "HI"), help="scale uniform in [LO, HI]")
    p.add_argument("--affine_shear", type=float, default=0.0, help="shear along x uniform in +-degrees")
    p.add_argument("--clahe", action="store_true", help="CLAHE contrast equalisation of the uint8 image (GPU, every mode)")
    p.add_argument("--clahe_grid", type=int, nargs=2, default=[8, 8], metavar=("GY", "GX"), help="tiles per axis, each 1..16, dividing the crop size")
    p.add_argument("--clahe_clip", type=float, default=2.0, metavar="C", help="clip limit in multiples of the mean bin height (0: no clipping)")
    p.add_argument("--mixup", type=float, default=0.0, metavar="ALPHA", help="Mixup of the uint8 batch at lambda ~ Beta(ALPHA, ALPHA) (GPU, training only; 0: off)")
    p.add_argument("--cutmix", type=float, default=0.0, metavar="ALPHA", help="CutMix of the uint8 batch at lambda ~ Beta(ALPHA, ALPHA) (GPU, training only; 0: off)")
    p.add_argument("--mix_prob", type=float, default=1.0, metavar="P", help="probability that a minibatch (--mix_mode elem: an image) is mixed")
    p.add_argument("--mix_switch_prob", type=float, default=0.5, metavar="P", help="probability of CutMix where --mixup and --cutmix are both on")
    p.add_argument("--mix_mode", default="batch", choices=["batch", "elem"], help="one lambda / box per minibatch, or per image")
    p.add_argument("--erase_prob", type=float, default=0.0, metavar="P", help="random erasing of the uint8 batch: probability per image (GPU, training only; 0: off)")
    p.add_argument("--erase_fill", type=int, default=136, metavar="V", help="grey level 0..255 an erased rectangle gets (default: the dataset mean)")
    p.add_argument("--uncertain", default="ones", choices=list(UNCERTAIN_POLICIES), help="policy for the uncertain (-1) training labels")
    p.add_argument("--pos_weight", nargs="+", default=None, metavar="W", help="`auto` or n_classes floats: positive-term weights of the loss")
    p.add_argument("--loss", default="bce", choices=["bce", "aucm", "focal", "asl", "hier"],
                   help="training loss: cross-entropy, the AUC min-max-margin loss, the focal loss, the asymmetric loss or the hierarchical "
                        "label loss (the evaluation loss written to eval_results stays the cross-entropy, comparable across training losses)")
    p.add_argument("--labels", default="competition", choices=["competition", "all"],
                   help="the findings read from the csv: the five competition labels, or all 14 in the csv's column order (sets --n_classes 14)")
    p.add_argument("--hier_mode", default=None, choices=["conditional", "unconditional"],
                   help="with --loss hier: the cross-entropy of each conditional logit where the ancestors are positive (default), or of "
                        "the product of probabilities along the path from the root")
    p.add_argument("--hier_parents", nargs="+", default=None, metavar="P",
                   help="with --loss hier: `auto` (default: the CheXpert tree, needs --labels all) or n_classes integers, the index of "
                        "each label's parent, -1 for a root, parents before children")
    p.add_argument("--no_hier_closure", action="store_true",
                   help="with --loss hier: leave the label tables as they are (default: a positive child makes its ancestors positive)")
    p.add_argument("--focal_gamma", type=float, default=None, metavar="G", help="focusing exponent of --loss focal (>= 0; default 2)")
    p.add_argument("--focal_alpha", type=float, default=None, metavar="A", help="class balance of --loss focal, in (0, 1) (default: none)")
    p.add_argument("--asl_gamma_pos", type=float, default=None, metavar="GP", help="positives' exponent of --loss asl (>= 0; default 0)")
    p.add_argument("--asl_gamma_neg", type=float, default=None, metavar="GN", help="negatives' exponent of --loss asl (>= 0; default 4)")
    p.add_argument("--asl_clip", type=float, default=None, metavar="M", help="probability shift of the negatives of --loss asl, in [0, 1) (default 0.05)")
    p.add_argument("--aucm_margin", type=float, default=None, metavar="M", help="margin of --loss aucm (> 0; default 1.0)")
    p.add_argument("--aucm_prior", nargs="+", default=None, metavar="P", help="`auto` (default) or n_classes positive rates in (0, 1) for --loss aucm")
    p.add_argument("--aucm_lr_aux", type=float, default=None, metavar="R", help="rate of the auxiliary scalars of --loss aucm (default: --lr)")
    p.add_argument("--synthetic_uncertain", type=float, default=0.0, metavar="F", help="fraction of the synthetic training labels marked uncertain")
    p.add_argument("--cam_classes", nargs="*", default=None, metavar="CLASS",
                   help="with --visualize: class-specific maps (gradcam.class_cam) of these class indices; no value or `all` = every class")
    p.add_argument("--saliency", default=None, choices=list(SALIENCY_METHODS), help="with --visualize: pixel attribution maps of the 'vis' subset")
    p.add_argument("--saliency_classes", nargs="*", default=None, metavar="CLASS", help="class indices of --saliency; no value or `all` = every class (default)")
    p.add_argument("--saliency_steps", type=int, default=None, metavar="M", help="path steps of ig (default 32) / noise samples of smoothgrad (default 16)")
    p.add_argument("--saliency_sigma", type=float, default=None, metavar="S", help="noise of smoothgrad in whitened units (default: 0.15 of the uint8 range)")
    p.add_argument("--saliency_baseline", default=None, choices=["mean", "black"], help="baseline of ig: the dataset mean grey (default) or black")
    p.add_argument("--saliency_chunk", type=int, default=None, metavar="R", help="rows per forward + backward pass of --saliency")
    p.add_argument("--clip_grad_norm", type=float, default=None, metavar="X", help="global-norm gradient clipping in the fused optimiser step")
    p.add_argument("--skip_nonfinite", action="store_true", help="drop the update of a minibatch whose gradient is not finite")
    p.add_argument("--ema_decay", type=float, default=None, metavar="D", help="exponential moving average of the weights, decay D in (0, 1)")
    p.add_argument("--no_ema_warmup", action="store_true", help="constant EMA decay (default: min(D, (1 + step) / (10 + step)))")
    p.add_argument("--use_ema", action="store_true", help="evaluate / visualise with the checkpoint's ema_state_dict")
    p.add_argument("--weight_decay", type=float, default=None, metavar="W", help="weight decay of the fused optimiser (>= 0)")
    p.add_argument("--decoupled_decay", action="store_true", help="decay the weights directly (AdamW's rule) instead of through the gradient")
    p.add_argument("--no_decay_norm_bias", action="store_true", help="no weight decay on 1-D parameters (BatchNorm, biases)")
    p.add_argument("--head_lr_mult", type=float, default=None, metavar="M", help="learning-rate multiplier of the classifier (the last nn.Linear)")
    p.add_argument("--backbone_lr_mult", type=float, default=None, metavar="M", help="learning-rate multiplier of everything but the classifier")
    p.add_argument("--freeze_backbone_steps", type=int, default=0, metavar="N",
                   help="train the classifier alone for the first N minibatches (-1: the whole run)")
    p.add_argument("--optimizer", default=None, choices=["lamb", "lars"],
                   help="layer-wise trust-ratio optimiser instead of the model's own (needs --fused_optimizer)")
    p.add_argument("--trust_coef", type=float, default=None, metavar="C", help="with --optimizer lars: the trust coefficient > 0 (default 0.001)")
    p.add_argument("--trust_clip", action="store_true", help="with --optimizer: trust ratios capped at 1")
    p.add_argument("--always_adapt", action="store_true", help="with --optimizer: adapt the tensors without weight decay too")
    p.add_argument("--sam_rho", type=float, default=None, metavar="R",
                   help="sharpness-aware minimisation around the fused optimiser with neighbourhood radius R > 0 (needs --fused_optimizer)")
    p.add_argument("--sam_adaptive", action="store_true", help="with --sam_rho: the scale-invariant form (ASAM)")
    p.add_argument("--bootstrap", type=int, default=0, metavar="B", help="bootstrap replicates of the AUROC intervals written beside every eval_results file (0: none)")
    p.add_argument("--bootstrap_seed", type=int, default=None, metavar="S", help="seed of the bootstrap draws (default: --seed)")
    p.add_argument("--bootstrap_unit", default="image", choices=list(BOOTSTRAP_UNITS), help="what the bootstrap resamples")
    p.add_argument("--bootstrap_alpha", type=float, default=0.05, metavar="A", help="the intervals cover 1 - A (default 0.05)")
    p.add_argument("--delong", action="store_true", default=False,
                   help="DeLong / Obuchowski AUROC intervals into delong_<tag>.json beside every eval_results file; paired test under --evaluate_ensemble")
    p.add_argument("--bootstrap_metrics", nargs="+", default=None, metavar="M",
                   help="with --bootstrap: intervals of these metrics (auroc, ap, sens@S, spec@S) into metrics_ci_<tag>.json")
    p.add_argument("--calibrate", default=None, choices=["temperature", "platt"],
                   help="fit a per-class calibration map on every evaluation's logits and write calibration_<tag>.json beside its results "
                        "(before / after on the fitting split itself is optimistic)")
    p.add_argument("--calibrate_smooth", action="store_true", help="with --calibrate: Platt's smoothed targets")
    p.add_argument("--calibration_from", default=None, metavar="FILE",
                   help="apply the fit stored in FILE (e.g. fitted on another split) instead of fitting; exclusive with --calibrate, whose "
                        "before / after on the fitting split itself is optimistic")
    p.add_argument("--calibration_bins", type=int, default=None, metavar="M",
                   help="bins of ECE / MCE and of the reliability diagram (1 .. 64, default 15); alone: the uncalibrated metrics only")
    p.add_argument("--calibration_binning", default="width", choices=["width", "mass"], help="equal-width or equal-mass bins")
    p.add_argument("--pool", default=None, choices=["avg", "max", "lse", "gem"],
                   help="global pooling in front of the classifier (FusedNet.set_pool; default: the checkpoint's, else the average): the "
                        "maximum, log-sum-exp with sharpness --pool_r, or the generalised mean with the trained exponent --pool_p")
    p.add_argument("--pool_r", type=float, default=None, metavar="R", help="with --pool lse: the sharpness r > 0 (default 10)")
    p.add_argument("--pool_p", type=float, default=None, metavar="P", help="with --pool gem: the exponent's start in [1, 16] (default 3)")
    p.add_argument("--head", default=None, choices=["linear", "csra", "pcam"],
                   help="head of the network (FusedNet.set_head; default: the checkpoint's, else linear): csra applies the classifier at "
                        "every pixel and pools the score map per class (class-specific residual attention); pcam pools it with the "
                        "per-pixel probabilities as weights (probabilistic-CAM pooling) and gives per-class probability maps")
    p.add_argument("--csra_lambda", type=float, default=None, metavar="L", help="with --head csra: the attention term's weight >= 0 (default 0.1)")
    p.add_argument("--csra_T", type=float, default=None, metavar="T", help="with --head csra: the softmax temperature > 0 (default 1)")
    p.add_argument("--pretrain", default=None, choices=["contrastive", "barlow"],
                   help="pretraining on two augmented views of every image instead of the supervised loss: contrastive (NT-Xent / SupCon) or barlow (Barlow Twins)")
    p.add_argument("--barlow_lambda", type=float, default=None, metavar="L", help="with --pretrain barlow: weight of the off-diagonal term, >= 0 (default 0.0051)")
    p.add_argument("--proj_dim", type=int, default=None, metavar="D", help="with --pretrain: width of the projection, the classifier nn.Linear (default 128; 512 under barlow)")
    p.add_argument("--temperature", type=float, default=None, metavar="T", help="with --pretrain: temperature of the contrastive loss, > 0 (default 0.2)")
    p.add_argument("--positive", default=None, choices=["view", "study", "patient"],
                   help="with --pretrain: what counts as a positive -- the other view of the image (default), or every row of its study / patient")
    p.add_argument("--knn_probe", type=int, default=None, metavar="K",
                   help="with --pretrain contrastive or --evaluate_single_model: the weighted kNN probe of the pooled features, K neighbours (1 .. 256)")
    p.add_argument("--knn_temperature", type=float, default=None, metavar="T", help="with --knn_probe: temperature of the vote's weights exp(s / T), > 0 (default 0.1)")
    p.add_argument("--knn_bank", type=int, default=None, metavar="N",
                   help="with --knn_probe: the bank is N training images at an even stride (default 8192); 0 = the whole training set")
    p.add_argument("--linear_probe", action="store_true",
                   help="with --pretrain contrastive or --evaluate_single_model: the linear probe, logistic regression fitted on the pooled features")
    p.add_argument("--probe_l2", type=float, nargs="+", default=None, metavar="L",
                   help="with --linear_probe: the L2 penalties of the fit, each >= 0 (default 0.001); one report entry per value")
    p.add_argument("--probe_bank", type=int, default=None, metavar="N",
                   help="with --linear_probe: the bank is N training images at an even stride (default 8192); 0 = the whole training set")
    p.add_argument("--probe_max_iter", type=int, default=None, metavar="I", help="with --linear_probe: L-BFGS iterations per class, >= 1 (default 200)")
    p.add_argument("--probe_save", default=None, metavar="FILE",
                   help="with --linear_probe, --evaluate_single_model and one --probe_l2: write a checkpoint whose classifier is the fit")
    p.add_argument("--init_backbone", default=None, metavar="FILE",
                   help="with --train: load every tensor of FILE's state_dict but the classifier's before the first step (exclusive with --restore)")
    p.add_argument("--num_workers", type=int, default=int(os.environ.get("CHEXPERT_NUM_WORKERS", "16")), help="decode / crop worker processes of the training loader (chexpert.py:77: "
                   "16); 0 = in-process")
    p.add_argument("--cache_decoded", type=float, default=float(os.environ.get("CHEXPERT_CACHE_GB", "0")), metavar="GB",
                   help="keep the decoded / resized / cropped training images in host shared memory (up to GB gigabytes; the "
                        "reference's transform has no random step, so epochs after the first skip the JPEG decode)")
    return p


class SyntheticXrays(torch.utils.data.Dataset):
    """Decoded grey bytes (1,S,S) uint8 U{0..255} -- what PIL hands the reference's transform chain (chexpert.py:67-72) after
    resize / centre-crop -- with Bernoulli(0.3) U-Ones-like labels (dataset.py:139-142).  uncertain_frac > 0: a second hash draw,
    independent of the labels', marks that fraction of them uncertain (-1), and the policy `uncertain` (data.apply_uncertain)
    then says what they become; 0 leaves the labels as they were, bit for bit."""

    def __init__(self, n, size, n_classes, seed, uncertain_frac=0.0, uncertain="ones"):
        self.n, self.size, self.n_classes, self.seed = n, size, n_classes, seed
        self.targets = synth.targets(seed + 1, n, n_classes)
        if uncertain_frac > 0:
            lab = self.targets.numpy().copy()
            lab[synth.uniform01(seed * 7919 + 104729, n * n_classes).reshape(n, n_classes) < uncertain_frac] = -1.0
            self.targets = torch.from_numpy(apply_uncertain(lab, uncertain, seed))

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return synth.xray_u8(self.seed * 1000003 + i, 1, self.size)[0], self.targets[i], i


def batches(ds, indices, batch_size, drop_last):
    for k in range(0, len(indices), batch_size):
        idx = indices[k:k + batch_size]
        if drop_last and len(idx) < batch_size:
            return
        items = [ds[i] for i in idx]
        yield torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items]), torch.tensor(idx)


def parse_args(argv=None):
    """The command line, --load_config applied, and what can be refused before anything is built refused here (parser.error): a
    --clahe grid that does not divide the crop size is an argument error, not a kernel status; so are the ranges of the sample-mixing
    flags and their combination with --loss aucm."""
    parser = build_parser()
    n_default = parser.get_default("n_classes")
    parser.set_defaults(n_classes=None)            # (so that a --n_classes that was given can contradict --labels all)
    args = parser.parse_args(argv)
    if args.load_config:
        args.__dict__.update(json.load(open(args.load_config)))
    if getattr(args, "labels", "competition") == "all":
        from .data import ATTR_NAMES_ALL
        if args.n_classes not in (None, len(ATTR_NAMES_ALL)):
            parser.error("--labels all reads the %d findings of the csv: --n_classes %d contradicts it" % (len(ATTR_NAMES_ALL), args.n_classes))
        args.n_classes = len(ATTR_NAMES_ALL)
    elif args.n_classes is None:
        args.n_classes = n_default
    if getattr(args, "clahe", False):
        from .augment import check_clahe_grid, clahe_clip_count
        size = args.resize or 320
        try:
            check_clahe_grid(args.clahe_grid, size, size)
            clahe_clip_count(args.clahe_clip, 1, 1)
        except ValueError as e:
            parser.error("--clahe: %s" % e)
    for name in ("mixup", "cutmix"):
        v = getattr(args, name, 0.0)
        if not (v >= 0.0 and np.isfinite(v)):
            parser.error("--%s takes a Beta parameter >= 0 (got %r)" % (name, v))
    for name, dflt in (("mix_prob", 1.0), ("mix_switch_prob", 0.5), ("erase_prob", 0.0)):
        v = getattr(args, name, dflt)
        if not 0.0 <= v <= 1.0:
            parser.error("--%s takes a probability in [0, 1] (got %r)" % (name, v))
    if not 0 <= getattr(args, "erase_fill", 136) <= 255:
        parser.error("--erase_fill takes a grey level 0..255 (got %r)" % args.erase_fill)
    if getattr(args, "mix_mode", "batch") not in ("batch", "elem"):
        parser.error("--mix_mode takes batch or elem (got %r)" % args.mix_mode)
    if (getattr(args, "mixup", 0.0) > 0 or getattr(args, "cutmix", 0.0) > 0) and getattr(args, "loss", "bce") == "aucm":
        parser.error("--mixup / --cutmix cannot be combined with --loss aucm: that loss thresholds the targets at 0.5, a blended "
                     "label has no meaning there (--erase_prob leaves the labels alone and is allowed)")
    boot, alpha, unit = getattr(args, "bootstrap", 0), getattr(args, "bootstrap_alpha", 0.05), getattr(args, "bootstrap_unit", "image")
    if boot < 0:
        parser.error("--bootstrap takes a number of replicates >= 0 (got %r)" % boot)
    if not 0.0 < alpha < 1.0:
        parser.error("--bootstrap_alpha takes a level inside (0, 1) (got %r)" % alpha)
    if unit not in BOOTSTRAP_UNITS:
        parser.error("--bootstrap_unit takes one of %s (got %r)" % (", ".join(BOOTSTRAP_UNITS), unit))
    if (boot > 0 or getattr(args, "delong", False)) and unit != "image" and getattr(args, "synthetic", 0):
        parser.error("--bootstrap_unit %s groups the images by their file paths; --synthetic images have none (use image)" % unit)
    names = getattr(args, "bootstrap_metrics", None)
    if names is not None:
        if boot <= 0:
            parser.error("--bootstrap_metrics needs --bootstrap B > 0 (the number of replicates)")
        try:
            M.parse_boot_metrics(names)
        except ValueError as e:
            parser.error("--bootstrap_metrics: %s" % e)
    fit, stored, bins = getattr(args, "calibrate", None), getattr(args, "calibration_from", None), getattr(args, "calibration_bins", None)
    if fit is not None and stored is not None:
        parser.error("--calibrate fits a map and --calibration_from applies a stored one: give one of the two")
    if fit is not None and fit not in ("temperature", "platt"):
        parser.error("--calibrate takes temperature or platt (got %r)" % fit)
    if getattr(args, "calibrate_smooth", False) and fit is None:
        parser.error("--calibrate_smooth needs --calibrate (the smoothed targets belong to the fit)")
    if bins is not None and not 1 <= bins <= 64:
        parser.error("--calibration_bins takes 1 .. 64 bins (got %r)" % bins)
    if getattr(args, "calibration_binning", "width") not in ("width", "mass"):
        parser.error("--calibration_binning takes width or mass (got %r)" % args.calibration_binning)
    if stored is not None and not os.path.isfile(stored):
        parser.error("--calibration_from: no file %s" % stored)
    try:
        pool = resolve_pool(args)
    except ValueError as e:
        parser.error(str(e))
    why = visualize_needs_avg(args, pool["kind"] if pool else "avg")
    if why:
        parser.error(why)
    try:
        head = resolve_head(args, pool)
    except ValueError as e:
        parser.error(str(e))
    why = visualize_needs_linear(args, head["kind"] if head else "linear")
    if why:
        parser.error(why)
    return args


def report_name(tag, stem, ext=".json"):
    """File name of the report `stem` that goes with <tag>.json: eval_results_step_5, "auc_ci" -> auc_ci_step_5.json (stems: auc_ci,
    delong, metrics_ci, calibration, and reliability with ext ".png" for the figure).  It must not start with `eval_results`:
    --plot_roc reads every file with that prefix as a compute_metrics dictionary."""
    return stem + "_" + (tag[len("eval_results_"):] if tag.startswith("eval_results_") else tag) + ext


def unit_groups(unit, ds, flag="--bootstrap_unit", none="image"):
    """One unit id per row of `ds`, or None for the unit `none`: the study ('.../patientN/studyK', what data.extract_patient_ids
    returns) or the patient (that without its last path component)."""
    if unit == none:
        return None
    if not hasattr(ds, "data"):
        raise ValueError("%s %s groups the images by their file paths; this dataset has none (use %s)" % (flag, unit, none))
    from .data import extract_patient_ids
    ids = [str(v) for v in extract_patient_ids(ds, ds.data.index)]
    return np.array(ids if unit == "study" else [v.rsplit("/", 1)[0] for v in ids])


def positive_codes(unit, ds, by_label=False):
    """--positive: None for `view`, else one integer per image of `ds`, the index of its study or patient.  The array is indexed by the
    image's position in `ds` (what `batches` yields) or, with by_label, by the csv row label that `ds[i]` returns as its third item
    (what the training loader yields; the two differ for a filtered or re-indexed frame): a table as long as the largest label, -1
    where no image has the label (augment.contrastive_ids refuses such an id)."""
    groups = unit_groups(unit, ds, "--positive", "view")
    if groups is None:
        return None
    codes = np.unique(groups, return_inverse=True)[1].astype(np.int64)
    if not by_label:
        return codes
    labels = np.asarray(ds.data.index, dtype=np.int64)
    table = np.full(int(labels.max()) + 1, -1, dtype=np.int64)
    table[labels] = codes
    return table


def bootstrap_groups(args, ds):
    """One resampling-unit id per validation row, or None for --bootstrap_unit image."""
    return unit_groups(getattr(args, "bootstrap_unit", "image"), ds)


def _interval_options(args):
    """(seed, alpha, device, unit) as the four reports below take them: --bootstrap_seed (default --seed), --bootstrap_alpha, the
    device of --cuda and --bootstrap_unit."""
    seed = getattr(args, "bootstrap_seed", None)
    return (args.seed if seed is None else seed, getattr(args, "bootstrap_alpha", 0.05), "cuda:%d" % (args.cuda or 0),
            getattr(args, "bootstrap_unit", "image"))


def _print_auc_intervals(ci):
    """One `AUC [lo, hi]` line per class and for the mean."""
    for c, name in enumerate(class_names(len(ci["aucs"]))):
        print("  %-18s %.4f [%.4f, %.4f]" % (name, ci["aucs"][c], ci["lo"][c], ci["hi"][c]))
    print("  %-18s %.4f [%.4f, %.4f]" % ("mean", ci["mean_auc"]["point"], ci["mean_auc"]["lo"], ci["mean_auc"]["hi"]))


def write_auc_ci(args, tag, outputs, targets, groups=None):
    """With --bootstrap B > 0: AUROC intervals of the evaluation that wrote <tag>.json, into auc_ci_<...>.json beside it, and one
    `AUC [lo, hi]` line per class and for the mean.  Returns the path, or None (B = 0: nothing computed, allocated or written)."""
    n_boot = getattr(args, "bootstrap", 0)
    if n_boot <= 0:
        return None
    seed, alpha, device, unit = _interval_options(args)
    ci = M.bootstrap_auc(outputs, targets, n_boot=n_boot, seed=seed, groups=groups, alpha=alpha, device=device)
    ci["unit"] = unit
    print("AUC with %g %% bootstrap intervals (%d replicates over %d %s units):" % (100 * (1 - ci["alpha"]), n_boot, ci["n_units"], ci["unit"]))
    _print_auc_intervals(ci)
    path = os.path.join(args.output_dir, report_name(tag, "auc_ci"))
    json.dump(ci, open(path, "w"), indent=4)
    return path


def write_delong(args, tag, outputs, targets, groups=None, members=None):
    """With --delong: the DeLong (Obuchowski with grouped units) AUROC intervals of the evaluation that wrote <tag>.json, into
    delong_<...>.json beside it, and one `AUC [lo, hi]` line per class and for the mean.  members: {checkpoint file name: that member's
    outputs} under --evaluate_ensemble; the file then holds under "vs_members" the paired test of `outputs` against each of them, and
    the mean-AUROC delta, z and p of each are printed.  Returns the path, or None (no --delong: nothing computed, allocated or written)."""
    if not getattr(args, "delong", False):
        return None
    _, alpha, device, unit = _interval_options(args)
    ci = M.delong_auc(outputs, targets, groups=groups, alpha=alpha, device=device)
    ci["unit"] = unit
    print("AUC with %g %% %s intervals (%d %s units):" % (100 * (1 - ci["alpha"]), ci["method"], ci["n_units"], ci["unit"]))
    _print_auc_intervals(ci)
    if members is not None:
        ci["vs_members"] = {}
        for name, out in members.items():
            d = M.delong_auc_diff(outputs, out, targets, groups=groups, alpha=alpha, device=device)
            ci["vs_members"][name] = d
            print("  ensemble - %-24s mean AUC delta %+.4f  z %.3f  p %.4g" % (name, d["mean_auc"]["delta"], d["mean_auc"]["z"], d["mean_auc"]["p"]))
    path = os.path.join(args.output_dir, report_name(tag, "delong"))
    json.dump(ci, open(path, "w"), indent=4)
    return path


def write_metrics_ci(args, tag, outputs, targets, groups=None):
    """With --bootstrap B > 0 and --bootstrap_metrics: the intervals of the named metrics of the evaluation that wrote <tag>.json, into
    metrics_ci_<...>.json beside it ({name: summary}), and one line per metric.  Returns the path, or None (nothing computed or written)."""
    n_boot, names = getattr(args, "bootstrap", 0), getattr(args, "bootstrap_metrics", None)
    if n_boot <= 0 or not names:
        return None
    seed, alpha, device, unit = _interval_options(args)
    ci = M.bootstrap_metrics(outputs, targets, metrics=names, n_boot=n_boot, seed=seed, groups=groups, alpha=alpha, device=device)
    for name, r in ci.items():
        r["unit"] = unit
        print("%s, mean over the classes: %.4f [%.4f, %.4f]" % (name, r["mean_auc"]["point"], r["mean_auc"]["lo"], r["mean_auc"]["hi"]))
    path = os.path.join(args.output_dir, report_name(tag, "metrics_ci"))
    json.dump(ci, open(path, "w"), indent=4)
    return path


def write_calibration(args, tag, outputs, targets, groups=None):
    """With --calibrate, --calibration_from or --calibration_bins: the calibration report of the evaluation that wrote <tag>.json, into
    calibration_<...>.json beside it -- the fit (fitted here or loaded), ECE / MCE / Brier and the reliability curves before and, where
    a map is applied, after it, with intervals under --bootstrap B -- and the figure reliability_<...>.png.  Returns the json's path, or
    None (none of the flags: nothing computed or written)."""
    method, stored, bins = getattr(args, "calibrate", None), getattr(args, "calibration_from", None), getattr(args, "calibration_bins", None)
    if method is None and stored is None and bins is None:
        return None
    from . import calibration as K
    from . import vis
    seed, alpha, device, unit = _interval_options(args)
    kw = dict(bins=15 if bins is None else bins, binning=getattr(args, "calibration_binning", "width"), n_boot=getattr(args, "bootstrap", 0),
              seed=seed, groups=groups, alpha=alpha, device=device)
    fit = None
    if method is not None:
        fit = K.fit_calibration(outputs, targets, method=method, smooth=getattr(args, "calibrate_smooth", False), device=device)
    elif stored is not None:
        fit = K.load_calibration(stored)
    report = {"fit": fit, "fitted_here": method is not None, "unit": unit}
    before = K.calibration_metrics(outputs, targets, None, **kw)
    report.update({"ece_before": before["ece"], "mce_before": before["mce"], "brier_before": before["brier"],
                   "reliability_before": before["reliability"]})
    after = None
    if fit is not None:
        after = K.calibration_metrics(outputs, targets, fit, **kw)
        report.update({"ece_after": after["ece"], "mce_after": after["mce"], "brier_after": after["brier"],
                       "reliability_after": after["reliability"]})
    for name in ("ece", "mce", "brier"):
        vals = [np.nanmean(list(r[name]["point"].values())) if r is not None and len(r[name]["point"]) else float("nan") for r in (before, after)]
        print("%s, mean over the classes: %.4f%s" % (name, vals[0], "" if after is None else " -> %.4f after the map" % vals[1]))
    path = os.path.join(args.output_dir, report_name(tag, "calibration"))
    json.dump(report, open(path, "w"), indent=4)
    vis.reliability_diagram(before["reliability"], class_names(len(before["ece"]["point"])),
                            os.path.join(args.output_dir, report_name(tag, "reliability", ".png")),
                            after=None if after is None else after["reliability"])
    return path


def make_clahe(args):
    """The equalisation step (chexpert_amd/augment.py), or None without --clahe: then nothing is launched or allocated for it."""
    if not getattr(args, "clahe", False):
        return None
    from .augment import Clahe
    return Clahe(args.clahe_grid, args.clahe_clip)


def make_affine(args, rank, device):
    """The geometric augmentation of the training loop (chexpert_amd/augment.py), or None: only --train with --affine warps --
    validation, --evaluate and --visualize see the images as the loader decoded them."""
    if not (args.affine and args.train):
        return None
    from .augment import RandomAffine
    return RandomAffine(args.affine_degrees, args.affine_translate, args.affine_scale, args.affine_shear, rank, device)


def make_mix(args, rank, device):
    """The sample-mixing step of the training loop (chexpert_amd/augment.py: SampleMix), or None: only --train with --mixup,
    --cutmix or --erase_prob mixes -- validation, --evaluate, --visualize and predict never do."""
    if not args.train:
        return None
    from .augment import make_sample_mix
    return make_sample_mix(getattr(args, "mixup", 0.0), getattr(args, "cutmix", 0.0), getattr(args, "mix_prob", 1.0),
                           getattr(args, "mix_switch_prob", 0.5), getattr(args, "mix_mode", "batch"), getattr(args, "erase_prob", 0.0),
                           getattr(args, "erase_fill", 136), rank, device)


def resolve_pos_weight(spec, targets, n_classes):
    """--pos_weight as a list of n_classes floats, or None.  `auto`: per class (non-ignored negatives) / (positives) of the training
    targets on the host, soft labels counted by their value (t to the positives, 1 - t to the negatives), clamped to [1/16, 16]
    (a class without positives gets 16)."""
    if spec is None:
        return None
    spec = [spec] if isinstance(spec, str) else list(spec)
    if len(spec) == 1 and str(spec[0]) == "auto":
        t = np.asarray(targets, dtype=np.float64)
        live = t >= 0
        pos = np.where(live, t, 0.0).sum(0)
        neg = np.where(live, 1.0 - t, 0.0).sum(0)
        w = np.where(pos > 0, neg / np.maximum(pos, 1e-300), 16.0)
        return [float(v) for v in np.clip(w, 1.0 / 16, 16.0)]
    w = [float(v) for v in spec]
    if len(w) != n_classes:
        raise ValueError("--pos_weight takes `auto` or %d floats (got %d)" % (n_classes, len(w)))
    if not all(np.isfinite(v) and v > 0 for v in w):
        raise ValueError("--pos_weight takes finite weights > 0 (got %s)" % w)
    return w


def class_names(n_classes, labels="competition"):
    if labels == "all":
        from .data import ATTR_NAMES_ALL
        if n_classes == len(ATTR_NAMES_ALL):
            return list(ATTR_NAMES_ALL)
    return ATTR_NAMES[:n_classes] if n_classes <= len(ATTR_NAMES) else ["class %d" % i for i in range(n_classes)]


def resolve_aucm_prior(spec, targets, n_classes):
    """--aucm_prior as a list of n_classes floats in (0, 1).  None or `auto`: per class positives / live labels of the training
    targets on the host, with the loss's own split: live is t >= 0, positive is t >= 0.5 (a soft label falls on the side it came
    from).  A class whose prior is not inside (0, 1) -- no positive, no negative or no live label at all -- is refused by name: the
    loss weighs its two sides by p and 1 - p."""
    names = class_names(n_classes)
    spec = ["auto"] if spec is None else [spec] if isinstance(spec, str) else [str(v) for v in spec]
    if spec == ["auto"]:
        t = np.asarray(targets, dtype=np.float64)
        if t.ndim != 2 or t.shape[1] != n_classes:
            raise ValueError("--aucm_prior auto needs the (N, %d) training targets (got shape %s)" % (n_classes, t.shape))
        live, pos = (t >= 0).sum(0), (t >= 0.5).sum(0)
        for c in range(n_classes):
            if live[c] == 0 or pos[c] == 0 or pos[c] == live[c]:
                raise ValueError("--aucm_prior auto: class %d (%s) has %d positives among %d non-ignored training labels; the AUC-margin "
                                 "loss needs a prior inside (0, 1), i.e. both positives and negatives" % (c, names[c], pos[c], live[c]))
        return [float(v) for v in pos / live]
    try:
        pr = [float(v) for v in spec]
    except ValueError:
        raise ValueError("--aucm_prior takes `auto` or %d floats (got %s)" % (n_classes, spec))
    if len(pr) != n_classes:
        raise ValueError("--aucm_prior takes `auto` or %d floats (got %d)" % (n_classes, len(pr)))
    for c, v in enumerate(pr):
        if not 0.0 < v < 1.0:
            raise ValueError("--aucm_prior: class %d (%s) has prior %r; it must be inside (0, 1)" % (c, names[c], v))
    return pr


def aucm_options(args, world=1):
    """--loss / --aucm_* checked before anything runs: None for the cross-entropy, else {"margin", "lr_aux"} (the prior needs the
    training table: resolve_aucm_prior)."""
    loss = getattr(args, "loss", "bce")
    margin, prior, lr_aux = getattr(args, "aucm_margin", None), getattr(args, "aucm_prior", None), getattr(args, "aucm_lr_aux", None)
    if loss != "aucm":
        if prior is not None or lr_aux is not None or margin is not None:
            raise ValueError("--aucm_margin / --aucm_prior / --aucm_lr_aux belong to --loss aucm: pass it with them")
        return None
    margin = 1.0 if margin is None else margin
    if args.pos_weight is not None:
        raise ValueError("--loss aucm cannot be combined with --pos_weight: the class prior is this loss's weighting")
    if not margin > 0:
        raise ValueError("--aucm_margin takes a margin > 0 (got %r)" % margin)
    lr_aux = args.lr if lr_aux is None else lr_aux
    if not lr_aux > 0:
        raise ValueError("--aucm_lr_aux takes a rate > 0 (got %r)" % lr_aux)
    if world > 1:
        from .models._fused import AUCM_DATA_PARALLEL
        raise RuntimeError("--loss aucm: " + AUCM_DATA_PARALLEL % world)
    return {"margin": float(margin), "lr_aux": float(lr_aux)}


def focus_options(args):
    """--loss focal|asl and their flags checked before anything runs: None for the other losses, else the keywords of
    FusedNet.set_loss (kind and the numbers; the weights come from --pos_weight)."""
    loss = getattr(args, "loss", "bce")
    fg, fa = getattr(args, "focal_gamma", None), getattr(args, "focal_alpha", None)
    gp, gn, m = getattr(args, "asl_gamma_pos", None), getattr(args, "asl_gamma_neg", None), getattr(args, "asl_clip", None)
    if loss != "focal" and (fg is not None or fa is not None):
        raise ValueError("--focal_gamma / --focal_alpha belong to --loss focal: pass it with them")
    if loss != "asl" and (gp is not None or gn is not None or m is not None):
        raise ValueError("--asl_gamma_pos / --asl_gamma_neg / --asl_clip belong to --loss asl: pass it with them")
    if loss == "focal":
        fg = 2.0 if fg is None else fg
        if not (fg >= 0 and np.isfinite(fg)):
            raise ValueError("--focal_gamma takes a finite exponent >= 0 (got %r)" % fg)
        if fa is not None and not 0 < fa < 1:
            raise ValueError("--focal_alpha takes a class balance inside (0, 1) (got %r)" % fa)
        return {"kind": "focal", "gamma": float(fg), "alpha": None if fa is None else float(fa)}
    if loss == "asl":
        gp, gn, m = 0.0 if gp is None else gp, 4.0 if gn is None else gn, 0.05 if m is None else m
        for name, v in (("--asl_gamma_pos", gp), ("--asl_gamma_neg", gn)):
            if not (v >= 0 and np.isfinite(v)):
                raise ValueError("%s takes a finite exponent >= 0 (got %r)" % (name, v))
        if not 0 <= m < 1:
            raise ValueError("--asl_clip takes a probability shift in [0, 1) (got %r)" % m)
        return {"kind": "asl", "gamma_pos": float(gp), "gamma_neg": float(gn), "clip": float(m)}
    return None


def multiclass_options(args):
    """--uncertain multiclass checked before anything runs: whether the run trains (or evaluates) the three-way softmax head.  What
    has no meaning for it is refused by naming both flags."""
    if getattr(args, "uncertain", "ones") != "multiclass":
        return False
    loss, soft = getattr(args, "loss", "bce"), "the three-way softmax has no soft-target form (--erase_prob leaves the labels alone and is allowed)"
    refused = [("--loss %s" % loss, loss != "bce", "the three-way softmax is this policy's loss"),
               ("--pos_weight", getattr(args, "pos_weight", None) is not None, "it weights the positive term of a sigmoid loss"),
               ("--mixup", getattr(args, "mixup", 0.0) > 0, soft), ("--cutmix", getattr(args, "cutmix", 0.0) > 0, soft),
               ("--visualize", bool(getattr(args, "visualize", False)),
                "the class indices of the CAM and saliency tools are head outputs, three per finding")]
    for flag, on, why in refused:
        if on:
            raise ValueError("--uncertain multiclass cannot be combined with %s: %s" % (flag, why))
    return True


def hier_options(args):
    """--loss hier and its flags checked before anything runs: None for the other losses, else {"parent": the table as a list of
    ints, "mode": --hier_mode, None where it was not given (a restored checkpoint's mode fills it in, hier_for_checkpoint; the default
    'conditional' comes after that: hier_mode_of), "closure": whether the label tables get data.hierarchy_closure, "explicit":
    whether --hier_parents gave the table}.  What has no meaning for the loss is refused by naming both flags."""
    loss = getattr(args, "loss", "bce")
    mode, spec, keep = getattr(args, "hier_mode", None), getattr(args, "hier_parents", None), getattr(args, "no_hier_closure", False)
    if loss != "hier":
        if mode is not None or spec is not None or keep:
            raise ValueError("--hier_mode / --hier_parents / --no_hier_closure belong to --loss hier: pass it with them")
        return None
    soft = "a blended label is positive for no ancestor test and closed under no tree (--erase_prob leaves the labels alone and is allowed)"
    for flag, on, why in (("--uncertain multiclass", getattr(args, "uncertain", "ones") == "multiclass", "the three-way softmax is that policy's loss"),
                          ("--mixup", getattr(args, "mixup", 0.0) > 0, soft), ("--cutmix", getattr(args, "cutmix", 0.0) > 0, soft)):
        if on:
            raise ValueError("--loss hier cannot be combined with %s: %s" % (flag, why))
    spec = ["auto"] if spec is None else [spec] if isinstance(spec, str) else [str(v) for v in spec]
    if spec == ["auto"]:
        if getattr(args, "labels", "competition") != "all":
            raise ValueError("--loss hier with --hier_parents auto needs --labels all: the five competition labels have no relation among "
                             "them (pass --labels all for the CheXpert tree, or --hier_parents as %d integers)" % args.n_classes)
        from .data import CHEXPERT_PARENT
        parent = list(CHEXPERT_PARENT)
    else:
        try:
            parent = [int(v) for v in spec]
        except ValueError:
            raise ValueError("--hier_parents takes `auto` or %d integers (got %s)" % (args.n_classes, spec))
    from .ops import check_hier_parent
    parent = check_hier_parent("--hier_parents", parent, args.n_classes).tolist()
    return {"parent": parent, "mode": mode, "closure": not keep, "explicit": spec != ["auto"]}


def hier_mode_of(hier):
    """The mode of a run's hierarchical loss once a restored checkpoint has had its say: --hier_mode or the checkpoint's, else 'conditional'."""
    return hier["mode"] or "conditional"


def hier_for_checkpoint(hier, loss_state, path, train=False):
    """The hierarchical loss of a run against a checkpoint's `loss_state`: a checkpoint of --loss hier brings its parent table, its mode
    and whether its label tables were closed under the tree (`closure`, which the command line writes beside them; absent: they
    were).  A --hier_parents or a --hier_mode that contradicts what is stored is refused (ValueError); a run without --hier_mode takes
    the stored mode; a run that evaluates without --loss hier takes everything from the checkpoint (its logits are conditional ones
    and have to be collapsed, and its validation table is treated as that run's was).  Returns the run's options, a new dict where
    the checkpoint changed them."""
    if (loss_state or {}).get("kind") != "hier":
        return hier
    stored = [int(v) for v in torch.as_tensor(loss_state["parent"]).tolist()]
    mode = loss_state.get("mode") or "conditional"
    if hier is None:
        if train:
            raise ValueError("--restore %s: the checkpoint was trained with --loss hier: pass it (and its flags) to go on training" % path)
        return {"parent": stored, "mode": mode, "closure": bool(loss_state.get("closure", True)), "explicit": False}
    if hier["parent"] != stored:
        raise ValueError("--restore %s: the checkpoint was trained with the parent table %s, --hier_parents gives %s" % (path, stored, hier["parent"]))
    if hier["mode"] not in (None, mode):
        raise ValueError("--restore %s: the checkpoint was trained with --hier_mode %s, this run asks for --hier_mode %s" % (path, mode, hier["mode"]))
    return hier if hier["mode"] == mode else dict(hier, mode=mode)


def check_member_hier(hier, ck, name):
    """A member of --evaluate_ensemble against the run: every member's logits go through one collapse, so either the run has --loss hier
    and every member was trained with it on the run's table, or neither has."""
    trained = checkpoint_loss_kind(ck) == "hier"
    if trained != (hier is not None):
        raise ValueError("--evaluate_ensemble: %s was trained %s --loss hier, this run is %s it: pass --loss hier and its table with a "
                         "folder of such checkpoints, and only then" % (name, "with" if trained else "without", "with" if hier is not None else "without"))
    if trained:
        hier_for_checkpoint(hier, ck["loss_state"], name)


def init_backbone_options(args):
    """--init_backbone checked before anything runs: it belongs to a --train run, excludes --restore and names a file.  Returns the
    path, or None without the flag."""
    init = getattr(args, "init_backbone", None)
    if init is not None:
        if not args.train:
            raise ValueError("--init_backbone starts a training run from a pretrained backbone: pass --train with it")
        if args.restore:
            raise ValueError("--init_backbone and --restore are exclusive: one starts a run from a backbone, the other continues a run")
        if not os.path.isfile(init):
            raise ValueError("--init_backbone: no file %s" % init)
    return init


PRETRAIN_PROJ_DIM = {"contrastive": 128, "barlow": 512}         # the default --proj_dim of each kind


def pretrain_kind(pretrain):
    """'contrastive' or 'barlow' of a pretrain_options dict (the contrastive one has no "kind" entry), None for None."""
    return None if pretrain is None else pretrain.get("kind", "contrastive")


def pretrain_options(args, world=1):
    """--pretrain contrastive | barlow and its flags checked before anything runs: None without it; for contrastive {"proj_dim",
    "temperature" (None: a restored checkpoint's, else 0.2: temperature_of), "positive"}; for barlow {"kind": "barlow", "proj_dim",
    "lambd" (None: a restored checkpoint's, else 0.0051: lambda_of), "positive": "view"}.  What the step cannot be combined with is
    refused with a one-line reason (ValueError)."""
    proj, tau, positive = getattr(args, "proj_dim", None), getattr(args, "temperature", None), getattr(args, "positive", None)
    lambd = getattr(args, "barlow_lambda", None)
    kind = getattr(args, "pretrain", None)
    if kind is None:
        if proj is not None or tau is not None or positive is not None:
            raise ValueError("--proj_dim / --temperature / --positive belong to --pretrain contrastive: pass it with them")
        if lambd is not None:
            raise ValueError("--barlow_lambda belongs to --pretrain barlow: pass it with it")
        return None
    from ._lib import NTXENT_MAX_D, NTXENT_MAX_N
    from .loss import check_lambda, check_temperature

    def no(flag, why):
        raise ValueError("--pretrain %s cannot be combined with %s: %s" % (kind, flag, why))
    if kind == "barlow":
        if tau is not None:
            no("--temperature", "the Barlow Twins loss has none (its one number is --barlow_lambda)")
        if positive not in (None, "view"):
            no("--positive %s" % positive, "the loss pairs the two views of an image and has no notion of several positives")
    elif lambd is not None:
        no("--barlow_lambda", "it belongs to --pretrain barlow")
    if not args.train:
        raise ValueError("--pretrain %s is a training mode: pass --train with it" % kind)
    for flag in ("evaluate_single_model", "evaluate_ensemble", "visualize", "plot_roc"):
        if getattr(args, flag, False):
            no("--" + flag, "the head is a projection, not a classifier: there are no findings to score or draw")
    if not (args.affine or args.jitter):
        raise ValueError("--pretrain %s needs --affine or --jitter (or both): without a random step the two views of an image are identical" % kind)
    if getattr(args, "mixup", 0.0) > 0 or getattr(args, "cutmix", 0.0) > 0 or getattr(args, "erase_prob", 0.0) > 0:
        no("--mixup / --cutmix / --erase_prob", "they mix or blank rows of the batch, whose labels the contrastive step does not read")
    if getattr(args, "loss", "bce") != "bce":
        no("--loss %s" % args.loss, "the contrastive loss is the step's loss")
    if getattr(args, "pos_weight", None) is not None:
        no("--pos_weight", "the labels are not read")
    if getattr(args, "uncertain", "ones") == "multiclass":
        no("--uncertain multiclass", "its head of three outputs per finding is a classifier's, the contrastive head is a projection")
    if getattr(args, "head", None) in ("csra", "pcam"):
        no("--head %s" % args.head, "the projection is the linear head")
    if world > 1:
        no("more than one rank (world size %d)" % world, "each rank would contrast its own rows only; gathering embeddings is not built")
    proj = PRETRAIN_PROJ_DIM[kind] if proj is None else proj
    if not 1 <= proj <= NTXENT_MAX_D:                  # (BARLOW_MAX_D and BARLOW_MAX_N are the same caps)
        raise ValueError("--proj_dim takes 1 .. %d (got %r)" % (NTXENT_MAX_D, proj))
    if 2 * args.batch_size > NTXENT_MAX_N:
        raise ValueError("--pretrain %s sees 2 x --batch_size rows per step, at most %d (got 2 x %d)" % (kind, NTXENT_MAX_N, args.batch_size))
    if kind == "barlow":
        if lambd is not None:
            check_lambda("--barlow_lambda", lambd)
        return {"kind": "barlow", "proj_dim": int(proj), "lambd": lambd, "positive": "view"}
    if tau is not None:
        check_temperature("--temperature", tau)
    positive = positive or "view"
    if positive != "view" and getattr(args, "synthetic", 0):
        raise ValueError("--positive %s groups the images by their file paths; --synthetic images have none (use view)" % positive)
    return {"proj_dim": int(proj), "temperature": tau, "positive": positive}


KNN_DEFAULT_T, KNN_DEFAULT_BANK = 0.1, 8192


def knn_options(args, world=1):
    """--knn_probe and its flags checked before anything runs: None without it, else {"k", "temperature", "bank"} (bank 0: the whole
    training set).  What the probe cannot run with is refused with a one-line reason (ValueError)."""
    k, T, bank = getattr(args, "knn_probe", None), getattr(args, "knn_temperature", None), getattr(args, "knn_bank", None)
    if k is None:
        if T is not None or bank is not None:
            raise ValueError("--knn_temperature / --knn_bank belong to --knn_probe K: pass it with them")
        return None
    from ._lib import KNN_MAX_K
    if getattr(args, "pretrain", None) is None and not getattr(args, "evaluate_single_model", False):
        raise ValueError("--knn_probe runs at the evaluations of --pretrain contrastive or with --evaluate_single_model: pass one of them")
    if world > 1:
        raise ValueError("--knn_probe cannot be combined with more than one rank (world size %d): gathering embeddings across ranks is "
                         "not built" % world)
    if not 1 <= k <= KNN_MAX_K:
        raise ValueError("--knn_probe takes 1 .. %d neighbours (got %r)" % (KNN_MAX_K, k))
    T = KNN_DEFAULT_T if T is None else T
    if not (T > 0 and np.isfinite(T)):
        raise ValueError("--knn_temperature must be finite and > 0 (got %r)" % (T,))
    bank = KNN_DEFAULT_BANK if bank is None else bank
    if bank < 0:
        raise ValueError("--knn_bank takes a number of training images >= 0, 0 being all of them (got %r)" % (bank,))
    if getattr(args, "head", None) in ("csra", "pcam"):
        raise ValueError("--knn_probe cannot be combined with --head %s: that head pools per-class score maps and has no pooled feature "
                         "vector" % args.head)
    return {"k": int(k), "temperature": float(T), "bank": int(bank)}


def knn_probe(run, embedded=None):
    """The kNN probe of run.model (knn.probe) under the run's deterministic preprocessing, as the dictionary the reports carry."""
    from . import knn
    o = run.knn
    return knn.probe(run.model, run.train_ds, run.valid_ds, o["k"], o["temperature"], o["bank"], run.args.batch_size, run.device, run.clahe,
                     embedded=embedded)


PROBE_DEFAULT_L2, PROBE_DEFAULT_MAX_ITER = 1e-3, 200


def probe_options(args, world=1):
    """--linear_probe and its flags checked before anything runs: None without it, else {"l2": [...], "bank", "max_iter", "save"} (bank
    0: the whole training set).  What the probe cannot run with is refused with a one-line reason (ValueError)."""
    on = getattr(args, "linear_probe", False)
    l2, bank = getattr(args, "probe_l2", None), getattr(args, "probe_bank", None)
    max_iter, save = getattr(args, "probe_max_iter", None), getattr(args, "probe_save", None)
    if not on:
        if l2 is not None or bank is not None or max_iter is not None or save is not None:
            raise ValueError("--probe_l2 / --probe_bank / --probe_max_iter / --probe_save belong to --linear_probe: pass it with them")
        return None
    if getattr(args, "pretrain", None) is None and not getattr(args, "evaluate_single_model", False):
        raise ValueError("--linear_probe runs at the evaluations of --pretrain contrastive or with --evaluate_single_model: pass one of them")
    if world > 1:
        raise ValueError("--linear_probe cannot be combined with more than one rank (world size %d): gathering embeddings across ranks "
                         "is not built" % world)
    if getattr(args, "head", None) in ("csra", "pcam"):
        raise ValueError("--linear_probe cannot be combined with --head %s: that head pools per-class score maps and has no pooled "
                         "feature vector" % args.head)
    if getattr(args, "uncertain", "ones") == "multiclass":
        raise ValueError("--linear_probe cannot be combined with --uncertain multiclass: its head has three logits per finding, the "
                         "probe fits one")
    if getattr(args, "loss", "bce") == "hier":
        raise ValueError("--linear_probe cannot be combined with --loss hier: its targets are conditional on the parent finding, the "
                         "probe fits one independent logit per finding")
    l2 = [PROBE_DEFAULT_L2] if l2 is None else [float(v) for v in l2]
    for v in l2:
        if not (v >= 0 and np.isfinite(v)):
            raise ValueError("--probe_l2 takes finite penalties >= 0 (got %r)" % (v,))
    bank = KNN_DEFAULT_BANK if bank is None else bank
    if bank < 0:
        raise ValueError("--probe_bank takes a number of training images >= 0, 0 being all of them (got %r)" % (bank,))
    max_iter = PROBE_DEFAULT_MAX_ITER if max_iter is None else max_iter
    if max_iter < 1:
        raise ValueError("--probe_max_iter takes a number of iterations >= 1 (got %r)" % (max_iter,))
    if save is not None:
        if not getattr(args, "evaluate_single_model", False):
            raise ValueError("--probe_save writes the evaluated checkpoint with the fitted classifier: pass --evaluate_single_model with it")
        if len(l2) != 1:
            raise ValueError("--probe_save takes the fit of exactly one --probe_l2 (got %d values)" % len(l2))
    return {"l2": l2, "bank": int(bank), "max_iter": int(max_iter), "save": save}


def run_probes(run):
    """(the kNN probe's report or None, the linear probe's or None) of run.model.  Where both are asked for and read the same bank, the
    two sets are embedded once.  The linear probe's report carries its fits under "_fits" (dropped before it is written)."""
    from . import knn, probe
    kn, lp = getattr(run, "knn", None), getattr(run, "probe", None)
    if kn is None and lp is None:
        return None, None
    sets = {}

    def embedded(n_bank):
        idx = knn.bank_indices(len(run.train_ds), n_bank)
        if len(idx) not in sets:
            sets[len(idx)] = (knn.embed_dataset(run.model, run.train_ds, idx, run.args.batch_size, run.device, run.clahe) +
                              knn.embed_dataset(run.model, run.valid_ds, range(len(run.valid_ds)), run.args.batch_size, run.device, run.clahe))
        return sets[len(idx)]

    knn_res = None if kn is None else knn_probe(run, embedded(kn["bank"]))
    lin_res = None if lp is None else probe.probe(run.model, run.train_ds, run.valid_ds, lp["l2"], lp["bank"], run.args.batch_size,
                                                  run.device, run.clahe, max_iter=lp["max_iter"], embedded=embedded(lp["bank"]))
    return knn_res, lin_res


def probe_report(res):
    """The linear probe's result as the reports carry it."""
    return {k: v for k, v in res.items() if not k.startswith("_")}


def print_probe(res, step):
    for f in res["fits"]:
        print("linear probe @ step %d: mean AUROC %.4f (l2 %g, bank %d, status %s, %d passes)\n%s" % (
            step, f["mean_auc"], f["l2"], res["bank"], "".join(str(s) for s in f["status"]), f["passes"], pprint.pformat(f["aucs"])))


def save_probe_checkpoint(run, res):
    """--probe_save: the model's weights with the classifier's two tensors replaced by the fit, the pooling's numbers, the source's
    step; no optimiser state and no loss_state (the probe is a BCE model whatever the backbone was trained with)."""
    fit, f = res["_fits"][0], res["fits"][0]
    sd = {k: v.detach().clone() for k, v in run.model.state_dict().items()}
    wk, bk = classifier_keys(run.model)
    sd[wk], sd[bk] = fit["W"].to(sd[wk].dtype), fit["b"].to(sd[bk].dtype)
    auc = f["mean_auc"]
    ckpt = {"global_step": run.args.step, "eval_loss": float(np.sum(f["train_loss"])), "avg_auc": 0.0 if np.isnan(auc) else float(auc),
            "state_dict": sd, "linear_probe": {"l2": f["l2"], "bank": res["bank"]}}
    if run.model.pool_kind != "avg":
        ckpt["pool_state"] = run.model.pool_state()
    folder = os.path.dirname(run.probe["save"])
    if folder:
        os.makedirs(folder, exist_ok=True)
    torch.save(ckpt, run.probe["save"])


def print_knn(res, step):
    print("kNN probe @ step %d: mean AUROC %.4f (k %d, T %g, bank %d)\n%s" % (step, res["mean_auc"], res["k"], res["temperature"], res["bank"],
                                                                           pprint.pformat(res["aucs"])))


def temperature_of(pretrain, restored_loss=None):
    """The temperature of a pretraining run: --temperature, else a restored checkpoint's, else 0.2."""
    if pretrain["temperature"] is not None:
        return float(pretrain["temperature"])
    return float((restored_loss or {}).get("temperature", 0.2))


def lambda_of(pretrain, restored_loss=None):
    """The lambda of a --pretrain barlow run: --barlow_lambda, else a restored checkpoint's, else 0.0051 (the paper's)."""
    if pretrain["lambd"] is not None:
        return float(pretrain["lambd"])
    return float((restored_loss or {}).get("lambd", 0.0051))


def check_checkpoint_pretrain(ck, pretrain, path, weight_key=None):
    """A checkpoint of --pretrain contrastive | barlow continues a run of its own kind and nothing else (its head is a projection: --init_backbone takes
    its backbone into a supervised run); a supervised checkpoint does not continue a pretraining run.  weight_key: the state_dict key
    of the classifier's weight (classifier_keys), whose rows are the checkpoint's --proj_dim."""
    stored = ck.get("pretrain")
    if stored is not None and pretrain is None:
        raise ValueError("--restore %s: the checkpoint is one of --pretrain %s, whose head is a projection: continue it with --pretrain "
                         "%s, or start a supervised run from its backbone with --init_backbone" % (path, stored, stored))
    if stored is None and pretrain is not None:
        raise ValueError("--restore %s: the checkpoint is a supervised one; --pretrain %s continues a pretraining run (its "
                         "backbone can start one: --init_backbone)" % (path, pretrain_kind(pretrain)))
    if stored is not None and stored != pretrain_kind(pretrain):
        raise ValueError("--restore %s: the checkpoint is one of --pretrain %s, this run is --pretrain %s: the two losses train "
                         "different projections (its backbone can start this run: --init_backbone)" % (path, stored, pretrain_kind(pretrain)))
    if stored is not None and weight_key is not None and weight_key in ck["state_dict"]:
        width = ck["state_dict"][weight_key].shape[0]
        if width != pretrain["proj_dim"]:
            raise ValueError("--restore %s: the checkpoint's projection has %d outputs, --proj_dim asks for %d" % (path, width, pretrain["proj_dim"]))


POOL_KEYS = ("pool_p", "pool_r")         # the pooling's own numbers: GeM's trained exponent, log-sum-exp's sharpness (FusedNet.set_pool)


def classifier_keys(model):
    """(weight, bias): the state_dict keys of the classifier, the last nn.Linear of every family."""
    last = [name for name, m in model.named_modules() if isinstance(m, nn.Linear)][-1]
    return last + ".weight", last + ".bias"


def backbone_state(model_sd, ckpt_sd, head_keys, path="", free=POOL_KEYS):
    """What --init_backbone loads: for every key of the model's state_dict outside `head_keys` the checkpoint's tensor.  A key the
    checkpoint lacks, one of another shape, or one the model has no place for is a ValueError that names it.  The keys of `free` --
    the pooling's numbers, which exist only under some --pool -- are taken where both sides hold them in one shape (a GeM exponent
    trained during pretraining goes on into a --pool gem run) and left alone otherwise: --pool stays free."""
    out = {}
    for k, v in model_sd.items():
        if k in head_keys:
            continue
        if k in free:
            if k in ckpt_sd and tuple(ckpt_sd[k].shape) == tuple(v.shape):
                out[k] = ckpt_sd[k]
            continue
        if k not in ckpt_sd:
            raise ValueError("--init_backbone %s: the checkpoint has no tensor %r (another --model?)" % (path, k))
        if tuple(ckpt_sd[k].shape) != tuple(v.shape):
            raise ValueError("--init_backbone %s: tensor %r has shape %s in the checkpoint, %s in this model"
                             % (path, k, tuple(ckpt_sd[k].shape), tuple(v.shape)))
        out[k] = ckpt_sd[k]
    for k in ckpt_sd:
        if k not in model_sd and k not in head_keys and k not in free:
            raise ValueError("--init_backbone %s: this model has no place for the checkpoint's tensor %r (another --model?)" % (path, k))
    return out


def init_backbone(model, path, device):
    """--init_backbone: the checkpoint's backbone (BatchNorm's running statistics included) into the model; the classifier, the step,
    the optimiser state and the loss state stay this run's.  Returns the keys loaded."""
    ck = torch.load(path, map_location=device)
    if not isinstance(ck, dict) or "state_dict" not in ck:
        raise ValueError("--init_backbone %s: not a checkpoint of this command line (no state_dict)" % path)
    own = model.state_dict()
    taken = backbone_state(own, ck["state_dict"], set(classifier_keys(model)), path)
    with torch.no_grad():
        for k, v in taken.items():
            own[k].copy_(v)
    return sorted(taken)


def head_width(args):
    """Outputs of the classifier: --n_classes findings, three logits each under --uncertain multiclass; under --pretrain contrastive
    the width of the projection, --proj_dim."""
    if getattr(args, "pretrain", None) is not None:
        return getattr(args, "proj_dim", None) or PRETRAIN_PROJ_DIM[args.pretrain]
    return args.n_classes * (3 if getattr(args, "uncertain", "ones") == "multiclass" else 1)


def checkpoint_loss_kind(ck):
    """The loss kind a checkpoint was trained with ('bce' where it carries no loss_state)."""
    return (ck.get("loss_state") or {}).get("kind", "bce")


def check_checkpoint_head(ck, multiclass, path):
    """A checkpoint of a --uncertain multiclass run has a head of three outputs per finding, every other one a head of one: the two do
    not load into each other, and the refusal says so before load_state_dict fails on a shape."""
    kind = checkpoint_loss_kind(ck)
    if (kind == "multiclass") != multiclass:
        raise ValueError("--restore %s: the checkpoint was trained %s --uncertain multiclass (loss kind %r), this run is %s it: the heads "
                         "differ (three outputs per finding against one)" % (path, "with" if kind == "multiclass" else "without", kind,
                                                                             "with" if multiclass else "without"))


def resolve_pool(args):
    """--pool / --pool_r / --pool_p checked before anything runs: None when --pool is absent (the checkpoint's pooling, else the
    average), or the keywords of FusedNet.set_pool.  --pool_r belongs to lse and --pool_p to gem (ValueError otherwise)."""
    from .pooling import DEFAULT_P, DEFAULT_R, check_pool
    kind, r, p = getattr(args, "pool", None), getattr(args, "pool_r", None), getattr(args, "pool_p", None)
    if r is not None and kind != "lse":
        raise ValueError("--pool_r is the sharpness of --pool lse: pass --pool lse with it")
    if p is not None and kind != "gem":
        raise ValueError("--pool_p is the exponent of --pool gem: pass --pool gem with it")
    if kind is None:
        return None
    try:
        kind, r, p = check_pool(kind, DEFAULT_R if r is None else r, DEFAULT_P if p is None else p)
    except ValueError as e:
        raise ValueError("--pool: %s" % e)
    return {"kind": kind, "r": r, "p": p}


def pool_for_checkpoint(pool, ck_pool):
    """The keywords of set_pool for a model that takes a checkpoint's weights: the checkpoint's `pool_state` (none: the average, a
    checkpoint from before the flag) decides the kind, and a --pool flag (`pool`: resolve_pool's dict, or None) that names another
    kind is refused -- before load_state_dict would fail on `pool_p` / `pool_r`.  r and p then come with the weights."""
    ck_kind = (ck_pool or {}).get("kind", "avg")
    if pool is not None and pool["kind"] != ck_kind:
        raise ValueError("--pool %s contradicts the checkpoint, which was trained with --pool %s: drop the flag, or pass the "
                         "checkpoint's" % (pool["kind"], ck_kind))
    out = {"kind": ck_kind}
    if ck_kind == "lse":
        out["r"] = (ck_pool or {}).get("r") or (pool or {}).get("r") or 10.0
    if ck_kind == "gem" and pool is not None:
        out["p"] = pool["p"]
    return out


def checkpoint_files(folder):
    """The checkpoint files of a folder, in the order every reader of it walks them (the members of --evaluate_ensemble)."""
    return sorted(f for f in os.listdir(folder) if f.startswith("checkpoint") and f.endswith(".pt"))


def restore_source(args):
    """(path, checkpoint) of the file --restore names, or of the first checkpoint of a folder, loaded to the CPU: what the model is
    shaped after before its weights are read (restore_pool, restore_head).  (None, None) without --restore or without such a file."""
    path = args.restore
    if path and os.path.isdir(path):
        files = checkpoint_files(path)
        path = os.path.join(path, files[0]) if files else None
    if not path or not os.path.isfile(path):
        return None, None
    return path, torch.load(path, map_location="cpu")


def restore_pool(args, pool, source=None):
    """What make_model hands set_pool: --pool without --restore; with --restore the pool_state of the checkpoint file (of the first
    checkpoint of a folder), checked against the flag (pool_for_checkpoint).  source: restore_source(args), where the caller has it."""
    _, ck = source or restore_source(args)
    if ck is None:
        return {k: v for k, v in (pool or {"kind": "avg"}).items() if v is not None}
    return pool_for_checkpoint(pool, ck.get("pool_state"))


def check_checkpoint_pool(ck, model, path):
    """A checkpoint whose pooling is not the model's is refused (ValueError) before load_state_dict."""
    kind = (ck.get("pool_state") or {}).get("kind", "avg")
    if kind != model.pool_kind:
        raise ValueError("checkpoint %s was trained with --pool %s, the model was built with --pool %s" % (path, kind, model.pool_kind))


def resolve_head(args, pool=None):
    """--head / --csra_lambda / --csra_T checked before anything runs: None when --head is absent (the checkpoint's head, else linear),
    or the keywords of FusedNet.set_head (lam / T None where the flag is absent: the checkpoint's, else the defaults).  The two numbers
    belong to --head csra, which stands on the average pool (`pool`: resolve_pool's dict); ValueError otherwise."""
    from .heads import DEFAULT_LAMBDA, DEFAULT_T, check_head
    kind, lam, T = getattr(args, "head", None), getattr(args, "csra_lambda", None), getattr(args, "csra_T", None)
    if (lam is not None or T is not None) and kind != "csra":
        raise ValueError("--csra_lambda and --csra_T belong to --head csra: pass --head csra with them")
    if kind is None:
        return None
    try:
        check_head(kind, DEFAULT_LAMBDA if lam is None else lam, DEFAULT_T if T is None else T)
    except ValueError as e:
        raise ValueError("--head: %s" % e)
    if kind != "linear" and pool is not None and pool["kind"] != "avg":
        raise ValueError("--head %s stands on the average pool: not with --pool %s" % (kind, pool["kind"]))
    return {"kind": kind, "lam": lam, "T": T}


def head_for_checkpoint(head, ck_head):
    """The keywords of set_head for a model that takes a checkpoint's weights.  The checkpoint's `head_state` (none: linear) names its
    head; --head linear on a csra checkpoint is refused.  --head csra on a linear checkpoint is the fine-tuning case (the keys are
    equal; lambda and T come from the command line).  On a csra checkpoint lambda and T are the checkpoint's unless the flags give them.
    --head pcam on a linear checkpoint is allowed in the same way (the keys are equal; the function changes); every other
    contradiction -- linear or csra on a pcam checkpoint, pcam on a csra one -- is refused."""
    from .heads import DEFAULT_LAMBDA, DEFAULT_T
    ck_head = ck_head or {}
    ck_kind = ck_head.get("kind", "linear")
    if head is not None and head["kind"] != ck_kind and ck_kind != "linear":
        raise ValueError("--head %s contradicts the checkpoint, which was trained with --head %s: drop the flag, or pass the "
                         "checkpoint's" % (head["kind"], ck_kind))
    kind = head["kind"] if head is not None else ck_kind
    if kind != "csra":
        return {"kind": kind}
    pick = lambda key, default: next(v for v in ((head or {}).get(key), ck_head.get(key), default) if v is not None)     # noqa: E731
    return {"kind": "csra", "lam": pick("lam", DEFAULT_LAMBDA), "T": pick("T", DEFAULT_T)}


def restore_head(args, head, pool_kind="avg", source=None):
    """What make_model hands set_head: --head without --restore; with --restore the head_state of the checkpoint file (of the first
    checkpoint of a folder), checked against the flag (head_for_checkpoint) and against the pooling.  source: restore_source(args), where the caller has it."""
    _, ck = source or restore_source(args)
    ck_head = ck.get("head_state") if ck is not None else None
    out = head_for_checkpoint(head, ck_head)
    if out["kind"] != "linear" and pool_kind != "avg":
        raise ValueError("--head %s stands on the average pool: the checkpoint pools with --pool %s" % (out["kind"], pool_kind))
    if out["kind"] == "pcam" and ck is not None and (ck_head or {}).get("kind", "linear") == "linear":
        print("--head pcam on a linear-head checkpoint: the weights load (the keys are equal), but the head computes another function "
              "of them (unlike --head csra at lambda 0): the first losses are not the checkpoint's")
    return out


def check_checkpoint_head_kind(ck, model, path):
    """A csra or pcam checkpoint is refused by a model with another head (ValueError); a linear checkpoint loads into every head (the
    keys are equal)."""
    kind = (ck.get("head_state") or {}).get("kind", "linear")
    if kind != "linear" and kind != model.head_kind:
        raise ValueError("checkpoint %s was trained with --head %s, the model was built with --head %s" % (path, kind, model.head_kind))


def visualize_needs_linear(args, kind):
    """Why --visualize cannot draw what was asked for on a model with head `kind` (None: it can).  Grad-CAM reads the head as pool +
    classifier; a csra or pcam model has its own maps (--cam_classes: heads.class_maps) and the saliency maps."""
    if kind == "linear" or not getattr(args, "visualize", False):
        return None
    if getattr(args, "cam_classes", None) is None and getattr(args, "saliency", None) is None:
        return ("--visualize draws Grad-CAM maps, which assume the linear head: with --head %s pass --cam_classes (its score and "
                "attention maps) or --saliency" % kind)
    return None


def visualize_needs_avg(args, kind):
    """Why --visualize cannot draw what was asked for on a model that pools with `kind` (None: it can).  Grad-CAM and the class
    maps read the head as an average; the saliency maps (--saliency) work with every pooling, and are then the only figures."""
    if kind == "avg" or not getattr(args, "visualize", False):
        return None
    if getattr(args, "cam_classes", None) is not None:
        return "--cam_classes draws class activation maps, which assume the average pool: not with --pool %s" % kind
    if getattr(args, "saliency", None) is None:
        return ("--visualize draws Grad-CAM maps, which assume the average pool: with --pool %s pass --saliency (pixel attribution works "
                "with every pooling)" % kind)
    return None


def resolve_cam_classes(spec, n_classes):
    """--cam_classes as a list of class indices, or None when the flag is absent.  No value or `all`: every class."""
    if spec is None:
        return None
    spec = [str(s) for s in spec]
    if not spec or spec == ["all"]:
        return list(range(n_classes))
    try:
        classes = [int(s) for s in spec]
    except ValueError:
        raise ValueError("--cam_classes takes class indices, `all` or no value (got %s)" % spec)
    if not all(0 <= c < n_classes for c in classes):
        raise ValueError("--cam_classes takes indices in [0, %d) (got %s)" % (n_classes, classes))
    return classes


SALIENCY_METHODS = ("grad", "smoothgrad", "smoothgrad_sq", "ig")


def resolve_saliency(args):
    """--saliency and its options as a dictionary {method, classes, steps, sigma, baseline, chunk}, or None when no --saliency* flag
    is given.  Refused here (ValueError), before anything is built: an option without --saliency, --saliency without --visualize, class
    indices out of range, steps or chunk <= 0, a negative sigma, an option that the method does not take."""
    method = getattr(args, "saliency", None)
    opts = {k: getattr(args, "saliency_" + k, None) for k in ("classes", "steps", "sigma", "baseline", "chunk")}
    given = [k for k, v in opts.items() if v is not None]
    if method is None:
        if given:
            raise ValueError("--saliency_%s belongs to --saliency METHOD: pass it too" % given[0])
        return None
    if method not in SALIENCY_METHODS:
        raise ValueError("--saliency takes one of %s (got %r)" % (", ".join(SALIENCY_METHODS), method))
    if not args.visualize:
        raise ValueError("--saliency draws attribution maps over the 'vis' subset: pass --visualize with it")
    try:
        classes = resolve_cam_classes(opts["classes"] if opts["classes"] is not None else [], args.n_classes)
    except ValueError as e:
        raise ValueError(str(e).replace("--cam_classes", "--saliency_classes")) from None
    steps = opts["steps"]
    if steps is not None and (method == "grad" or steps <= 0):
        raise ValueError("--saliency_steps takes a number >= 1 of path steps (ig) or noise samples (smoothgrad) (got %r with %s)" % (steps, method))
    if opts["sigma"] is not None and (not method.startswith("smoothgrad") or not opts["sigma"] >= 0):
        raise ValueError("--saliency_sigma is the noise >= 0 of smoothgrad / smoothgrad_sq (got %r with %s)" % (opts["sigma"], method))
    if opts["baseline"] is not None and method != "ig":
        raise ValueError("--saliency_baseline belongs to --saliency ig (got it with %s)" % method)
    if opts["chunk"] is not None and opts["chunk"] <= 0:
        raise ValueError("--saliency_chunk takes a number of rows >= 1 (got %r)" % opts["chunk"])
    return {"method": method, "classes": classes, "steps": steps if steps is not None else (32 if method == "ig" else 16),
            "sigma": opts["sigma"], "baseline": opts["baseline"] or "mean", "chunk": opts["chunk"]}


def saliency_maps(model, x, sal):
    """The (B,K,H,W) maps of --saliency for a whitened (B,3,H,W) batch on the GPU: grad, smoothgrad and smoothgrad_sq as the sum of
    the channels' magnitudes, ig signed (the sum over the channels, whose pixel sum is the completeness identity's left side)."""
    from . import saliency as S
    m, cl, ch = sal["method"], sal["classes"], sal["chunk"]
    if m == "grad":
        return S.input_gradient(model, x, cl, channels="abs")
    if m == "ig":
        return S.integrated_gradients(model, x, cl, steps=sal["steps"], baseline=None if sal["baseline"] == "mean" else "black", chunk=ch)[0]
    return S.smoothgrad(model, x, cl, samples=sal["steps"], sigma=sal["sigma"], squared=m == "smoothgrad_sq", chunk=ch)


def optimizer_options(args):
    """--clip_grad_norm / --skip_nonfinite / --ema_decay / --no_ema_warmup as keyword arguments of the fused optimisers ({}: all off)."""
    clip, skip, ema = getattr(args, "clip_grad_norm", None), getattr(args, "skip_nonfinite", False), getattr(args, "ema_decay", None)
    no_warm, use_ema = getattr(args, "no_ema_warmup", False), getattr(args, "use_ema", False)
    for flag, on in (("--clip_grad_norm", clip is not None), ("--skip_nonfinite", skip), ("--ema_decay", ema is not None),
                     ("--no_ema_warmup", no_warm)):
        if on and not args.fused_optimizer:
            raise ValueError("%s works inside the fused optimiser step: pass --fused_optimizer with it" % flag)
    if clip is not None and not clip > 0:
        raise ValueError("--clip_grad_norm takes a norm > 0 (got %r)" % clip)
    if ema is not None and not 0.0 < ema < 1.0:
        raise ValueError("--ema_decay takes a decay in (0, 1) (got %r)" % ema)
    if no_warm and ema is None:
        raise ValueError("--no_ema_warmup changes the decay of --ema_decay: pass --ema_decay D with it")
    if use_ema and args.train:
        raise ValueError("--use_ema picks the weights of --evaluate_single_model / --evaluate_ensemble / --visualize; training "
                         "evaluates with the average whenever --ema_decay is given")
    if clip is None and not skip and ema is None:
        return {}
    return {"max_grad_norm": clip, "skip_nonfinite": bool(skip), "ema_decay": ema, "ema_warmup": not no_warm}


def group_options(args):
    """--weight_decay / --decoupled_decay / --no_decay_norm_bias / --head_lr_mult / --backbone_lr_mult / --freeze_backbone_steps,
    validated: ({} when all are off, else the keyword arguments of optim.finetune_groups under "finetune" (None: no groups
    needed) plus "weight_decay" and "decoupled" for the optimiser's constructor and "freeze_steps")."""
    import math
    wd, dec = getattr(args, "weight_decay", None), getattr(args, "decoupled_decay", False)
    nd = getattr(args, "no_decay_norm_bias", False)
    hm, bm = getattr(args, "head_lr_mult", None), getattr(args, "backbone_lr_mult", None)
    fz = getattr(args, "freeze_backbone_steps", 0)
    for flag, on in (("--weight_decay", wd is not None), ("--decoupled_decay", dec), ("--no_decay_norm_bias", nd),
                     ("--head_lr_mult", hm is not None), ("--backbone_lr_mult", bm is not None), ("--freeze_backbone_steps", fz != 0)):
        if on and not args.fused_optimizer:
            raise ValueError("%s works inside the fused optimiser step: pass --fused_optimizer with it" % flag)
    if wd is not None and not (math.isfinite(wd) and wd >= 0):
        raise ValueError("--weight_decay takes a finite decay >= 0 (got %r)" % wd)
    for flag, v in (("--head_lr_mult", hm), ("--backbone_lr_mult", bm)):
        if v is not None and not (math.isfinite(v) and v >= 0):
            raise ValueError("%s takes a finite multiplier >= 0 (got %r)" % (flag, v))
    if fz < -1:
        raise ValueError("--freeze_backbone_steps takes a number of minibatches >= 0, or -1 for the whole run (got %r)" % fz)
    if (dec or nd) and not wd:
        raise ValueError("%s changes how --weight_decay is applied: pass --weight_decay W > 0 with it"
                         % ("--decoupled_decay" if dec else "--no_decay_norm_bias"))
    if wd is None and not dec and not nd and hm is None and bm is None and fz == 0:
        return {}
    finetune = None
    if nd or hm is not None or bm is not None or fz != 0:
        finetune = {"weight_decay": wd or 0.0, "no_decay_norm_bias": bool(nd), "head_lr_mult": 1.0 if hm is None else hm,
                    "backbone_lr_mult": 1.0 if bm is None else bm, "freeze_backbone": fz != 0}
    return {"weight_decay": wd or 0.0, "decoupled": bool(dec), "finetune": finetune, "freeze_steps": fz}


def trust_options(args):
    """--optimizer / --trust_coef / --trust_clip / --always_adapt, validated: {} without --optimizer (the model's own optimiser, as
    ever), else {"kind", "trust_clip", "always_adapt"} and, for lars, "trust_coef"."""
    import math
    kind, coef = getattr(args, "optimizer", None), getattr(args, "trust_coef", None)
    clip, adapt = getattr(args, "trust_clip", False), getattr(args, "always_adapt", False)
    if kind is None:
        for flag, on in (("--trust_coef", coef is not None), ("--trust_clip", clip), ("--always_adapt", adapt)):
            if on:
                raise ValueError("%s belongs to the trust-ratio optimisers: pass --optimizer lamb|lars with it" % flag)
        return {}
    if kind not in ("lamb", "lars"):
        raise ValueError("--optimizer takes lamb or lars (got %r)" % (kind,))
    if not args.fused_optimizer:
        raise ValueError("--optimizer %s works inside the fused optimiser step: pass --fused_optimizer with it" % kind)
    if getattr(args, "decoupled_decay", False):
        raise ValueError("--decoupled_decay cannot be combined with --optimizer %s: %s" % (kind, (
            "LAMB's weight decay already sits outside the moments" if kind == "lamb" else "LARS's weight decay is part of the trust ratio")))
    out = {"kind": kind, "trust_clip": bool(clip), "always_adapt": bool(adapt)}
    if coef is not None:
        if kind != "lars":
            raise ValueError("--trust_coef is the coefficient of --optimizer lars; lamb's ratio has none")
        if not (math.isfinite(coef) and coef > 0):
            raise ValueError("--trust_coef takes a finite coefficient > 0 (got %r)" % coef)
        out["trust_coef"] = float(coef)
    return out


def sam_options(args, world=1):
    """--sam_rho / --sam_adaptive, validated before anything runs: {} without --sam_rho, else {"rho", "adaptive"}."""
    import math
    rho, adaptive = getattr(args, "sam_rho", None), getattr(args, "sam_adaptive", False)
    if rho is None:
        if adaptive:
            raise ValueError("--sam_adaptive chooses the form of sharpness-aware minimisation: pass --sam_rho R with it")
        return {}
    if not args.fused_optimizer:
        raise ValueError("--sam_rho works around the fused optimiser step: pass --fused_optimizer with it")
    if not (math.isfinite(rho) and rho > 0):
        raise ValueError("--sam_rho takes a finite radius > 0 (got %r)" % rho)
    if getattr(args, "loss", "bce") == "aucm":
        raise ValueError("--sam_rho cannot be combined with --loss aucm: the auxiliary update of the AUC-margin loss runs inside the "
                         "fused step and would run twice")
    if world > 1:
        raise ValueError("--sam_rho is not supported on more than one rank (world size %d): the first pass would have to skip the "
                         "all-reduce" % world)
    return {"rho": float(rho), "adaptive": bool(adaptive)}


def trust_optimizer(args, model, tr):
    """(optimiser, scheduler) of --optimizer lamb|lars over `model`: FusedLAMB has no schedule, FusedLARS its parent's MultiStepLR."""
    from . import optim as O
    kw = dict(fused_optimizer_kwargs(args, model), **{k: v for k, v in tr.items() if k != "kind"})
    if tr["kind"] == "lamb":
        return O.FusedLAMB(model, lr=args.lr, **kw), None
    return O.FusedLARS(model, lr=args.lr, **kw), "fused"


def fused_optimizer_kwargs(args, model):
    """Keyword arguments of the fused optimiser's constructor for the clip / skip / EMA and the parameter-group flags."""
    from . import optim as O
    kw = dict(optimizer_options(args))
    go = group_options(args)
    if go:
        kw["weight_decay"] = go["weight_decay"]
        if go["decoupled"]:
            kw["decoupled"] = True
        if go["finetune"] is not None:
            kw["groups"] = O.finetune_groups(model, **go["finetune"])
    return kw


def thaw_backbone(optimizer):
    """--freeze_backbone_steps N, after minibatch N: the backbone's rows of the group table are rewritten on the device."""
    for i, name in enumerate(optimizer.group_names):
        if name.startswith("backbone"):
            optimizer.set_group(i, frozen=False)


def model_weights(ck, args, path=""):
    """The state dict a checkpoint is read for: the live weights, or with --use_ema (outside training) their average."""
    if getattr(args, "use_ema", False) and not args.train:
        if "ema_state_dict" not in ck:
            raise RuntimeError("--use_ema: checkpoint %s holds no ema_state_dict (it was not trained with --ema_decay)" % path)
        return ck["ema_state_dict"]
    return ck["state_dict"]


def make_model(args, device, pool=None, head=None):
    """`model_and_own_optimizer`, or with --optimizer lamb|lars the same model under that optimiser (every --model alike); with
    --sam_rho the optimiser is wrapped in optim.FusedSAM."""
    tr = trust_options(args)                                 # validated before a model is built
    sam = sam_options(args)
    model, opt, sched = model_and_own_optimizer(args, device, pool, head)
    if tr:
        opt, sched = trust_optimizer(args, model, tr)
    if sam:                                                  # around whichever fused optimiser the flags chose; same scheduler
        from . import optim as O
        opt = O.FusedSAM(opt, **sam)
    return model, opt, sched


def model_and_own_optimizer(args, device, pool=None, head=None):
    """Model zoo and optimiser wiring of chexpert.py:461-502.  pool: the keywords of FusedNet.set_pool (None: the average), applied
    before the optimiser is built -- GeM's exponent is one of its parameters.  head: the keywords of FusedNet.set_head (None: linear)."""
    from . import optim as O
    from .models import densenet121
    name = args.model
    fused = args.fused_optimizer
    optimizer_options(args)                                  # validated before a model is built
    group_options(args)
    n_out = head_width(args)                                 # (three logits per finding under --uncertain multiclass)
    size = args.resize or 320
    attn = {"k": 0.2, "v": 0.1, "nh": 8, "relative": True, "input_dims": (size, size)}
    # the bare module and the family of its own optimiser
    if name == "densenet121":
        model, own = densenet121(pretrained=args.pretrained), "adam"
        model.classifier = nn.Linear(model.classifier.in_features, n_out)
        nn.init.constant_(model.classifier.bias, 0)
    elif name in ("aadensenet121", "densenet121_attn_aug"):    # chexpert.py:474-480 (README row name accepted too)
        from .models import DenseNet
        model, own = DenseNet(32, (6, 12, 24, 16), 64, num_classes=n_out, attn_params=attn), "sgd"
    elif name == "resnet152":                                 # chexpert.py:481-486
        from .models import resnet152
        model, own = resnet152(pretrained=args.pretrained), "adam"
        model.fc = nn.Linear(model.fc.in_features, n_out)
    elif "efficientnet" in name:                              # chexpert.py:496-500
        from .models import construct_model
        model, own = construct_model(name, n_classes=n_out), "rmsprop"
    elif name == "aaresnet152":                               # chexpert.py:486-494
        from .models import Bottleneck, ResNet
        model, own = ResNet(Bottleneck, [3, 8, 36, 3], num_classes=n_out, attn_params=attn), "adam"
    else:
        raise RuntimeError("Model architecture not supported.")
    model = model.storage_dtype(args.dtype).to(device).set_pool(**(pool or {})).set_head(**(head or {}))
    if fused:
        kw = fused_optimizer_kwargs(args, model)             # the constructor's keyword arguments, now that `model` exists
        if own == "adam":
            return model, O.FusedAdam(model, lr=args.lr, **kw), None
        if own == "sgd":
            return model, O.FusedSGDNesterov(model, lr=args.lr, **kw), "fused"
        return model, O.FusedRMSprop(model, lr=args.lr, decay=args.lr_decay_factor, **kw), "fused"
    if own == "adam":
        return model, torch.optim.Adam(model.parameters(), lr=args.lr), None
    if own == "sgd":
        opt = torch.optim.SGD(model.parameters(), lr=args.lr, momentum=0.9, nesterov=True)
        return model, opt, torch.optim.lr_scheduler.MultiStepLR(opt, [40000, 60000])
    opt = torch.optim.RMSprop(model.parameters(), lr=args.lr, momentum=0.9, eps=0.001)
    return model, opt, torch.optim.lr_scheduler.ExponentialLR(opt, args.lr_decay_factor)


def collapse_of(collapse):
    """The function that makes (N, n_classes) binary logits of a forward's output: None where they are that already, for True the
    collapse of the three-way head (loss.collapse_multiclass), for a parent table that of the hierarchical loss's conditional
    logits (loss.collapse_hierarchy); a host table is checked here, once, and copied to a device with the first batch from it."""
    if collapse is None or collapse is False:
        return None
    if collapse is True:
        from .loss import collapse_multiclass
        return collapse_multiclass
    from .loss import collapse_hierarchy
    if isinstance(collapse, torch.Tensor) and collapse.is_cuda:
        return lambda o: collapse_hierarchy(o, collapse)
    from .ops import check_hier_parent
    table, on = check_hier_parent("collapse_of", collapse), {}

    def run(o):
        if o.device not in on:
            on[o.device] = table.to(o.device)
        return collapse_hierarchy(o, on[o.device])
    return run


@torch.no_grad()
def evaluate(model, ds, indices, batch_size, device, pre=None, collapse=False):
    """chexpert.py:198-211 on this rank's slice of the validation set; returns logits, targets, per-element losses, indices.
    `pre`: the deterministic preprocessing of the uint8 batch on the GPU (--clahe), or None.  `collapse`: the model has the three-way
    head of --uncertain multiclass; its logits become binary ones right after the forward (loss.collapse_multiclass), so everything
    from the element losses on sees (N, n_classes).  A parent table as `collapse`: the model was trained with --loss hier; its
    conditional logits become unconditional ones at the same place (loss.collapse_hierarchy)."""
    model.eval()
    outs, tgts, losses, ids = [], [], [], []
    loss_fn = nn.BCEWithLogitsLoss(reduction="none")
    if bool((ds.targets < 0).any()):               # ignored labels in this table: their element losses are 0 (cx_bce_masked_fwd_bwd)
        from .loss import MaskedBCE
        loss_fn = MaskedBCE().elementwise
    collapse = collapse_of(collapse)
    for x, t, idx in batches(ds, indices, batch_size, False):
        o = model(x.to(device) if pre is None else pre(x.to(device)))
        if collapse is not None:
            o = collapse(o)
        losses.append(loss_fn(o, t.to(device)))
        outs.append(o)
        tgts.append(t.to(device))
        ids.append(idx.to(device))
    if not outs:
        z = torch.zeros(0, ds.n_classes, device=device)
        return z, z.clone(), z.clone(), torch.zeros(0, dtype=torch.int64, device=device)
    return torch.cat(outs), torch.cat(tgts), torch.cat(losses), torch.cat(ids)


def evaluate_sharded(model, ds, batch_size, device, rank, world, pre=None, collapse=False):
    """Every rank forwards indices rank::world; the (N,5) logits / targets / losses are gathered and put back in dataset order."""
    idx = list(range(len(ds)))[rank::world]
    o, t, l, i = evaluate(model, ds, idx, batch_size, device, pre, collapse)
    o, t, l, i = (P.gather_rows(v) for v in (o, t, l, i))
    order = torch.argsort(i)
    return o[order].cpu(), t[order].cpu(), l[order].cpu()


def save_checkpoint(ckpt, optim_state, sched_state, args, max_records=10):
    """Latest + the `max_records` best checkpoints by mean AUROC with a tracker file
    (behaviour of chexpert.py:90-123: evict the lowest-AUROC record and re-use its file id)."""
    d = args.output_dir
    os.makedirs(os.path.join(d, "best_checkpoints"), exist_ok=True)
    torch.save(ckpt, os.path.join(d, "checkpoint_latest.pt"))
    torch.save(optim_state, os.path.join(d, "optim_checkpoint_latest.pt"))
    if sched_state:
        torch.save(sched_state, os.path.join(d, "sched_checkpoint_latest.pt"))
    path = os.path.join(d, "checkpoints_tracker.csv")
    recs = []
    if os.path.exists(path):
        recs = [list(r) for r in np.atleast_2d(np.loadtxt(path, skiprows=1))]
    file_id, floor = len(recs), float("-inf")
    if len(recs) == max_records:
        worst = min(range(len(recs)), key=lambda i: recs[i][3])
        floor, file_id = recs[worst][3], int(recs[worst][0])
        recs.pop(worst)
    recs.append([file_id, args.step, float(ckpt["eval_loss"]), float(ckpt["avg_auc"])])
    recs.sort(key=lambda r: -r[3])
    if ckpt["avg_auc"] > floor:
        np.savetxt(path, np.array(recs), delimiter=" ", header="CheckpointId Step Loss AvgAUC")
        torch.save(ckpt, os.path.join(d, "best_checkpoints", "checkpoint_%d.pt" % file_id))


def restore(args, model, optimizer, scheduler, device, multiclass=False, pretrain=None):
    """chexpert.py:504-518: model weights + step from the file; when training also `optim_<name>` / `sched_<name>` beside it.
    Returns the checkpoint's `loss_state` entry (FusedNet.loss_state() of a --loss aucm, focal or asl or --uncertain multiclass run),
    or None.  A checkpoint whose head is not this run's (`multiclass`) is refused (ValueError) before anything is loaded."""
    ck = torch.load(args.restore, map_location=device)
    check_checkpoint_pretrain(ck, pretrain, args.restore, classifier_keys(model)[0])
    check_checkpoint_head(ck, multiclass, args.restore)
    check_checkpoint_pool(ck, model, args.restore)
    check_checkpoint_head_kind(ck, model, args.restore)
    model.load_state_dict(model_weights(ck, args, args.restore))
    args.step = ck["global_step"]
    if args.train:
        d, b = os.path.dirname(args.restore), os.path.basename(args.restore)
        optimizer.load_state_dict(torch.load(os.path.join(d, "optim_" + b), map_location=device))
        if scheduler is not None and scheduler != "fused":
            scheduler.load_state_dict(torch.load(os.path.join(d, "sched_" + b), map_location=device))
    return ck.get("loss_state")


def plot_roc(res, args, name):
    """chexpert.py:399-427: ROC and precision-recall curves per class from an eval_results_*.json."""
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    n = len(res["aucs"])
    fig, axs = plt.subplots(2, n, figsize=(4 * n, 8))
    for i in range(n):
        k = str(i) if str(i) in res["fpr"] else i
        axs[0, i].plot(res["fpr"][k], res["tpr"][k], label="AUC = %.2f" % res["aucs"][k])
        axs[0, i].plot([0, 1], [0, 1], "k--")
        axs[0, i].set_xlabel("False positive rate")
        axs[0, i].set_ylabel("True positive rate")
        axs[0, i].set_title(ATTR_NAMES[i] if i < len(ATTR_NAMES) else "class %d" % i)
        axs[0, i].legend(loc="lower right")
        axs[1, i].step(res["recall"][k], res["precision"][k], where="post")
        axs[1, i].set_xlabel("Recall")
        axs[1, i].set_ylabel("Precision")
    plt.tight_layout()
    os.makedirs(os.path.join(args.output_dir, "plots"), exist_ok=True)
    plt.savefig(os.path.join(args.output_dir, "plots", name + ".png"), bbox_inches="tight")
    plt.close()


def check_flags(argv=None):
    """Phase 1: every refusal a flag can earn on its own, in a fixed order, before a process group, a directory or a dataset exists.
    Returns the run's container: `args`, rank / world / local and what the option families resolved to (None or empty: off)."""
    args = parse_args(argv)
    if not 0.0 <= args.synthetic_uncertain <= 1.0:
        raise ValueError("--synthetic_uncertain takes a fraction in [0, 1] (got %r)" % args.synthetic_uncertain)
    if args.synthetic_uncertain > 0 and not args.synthetic:
        raise ValueError("--synthetic_uncertain marks labels of the synthetic set: pass --synthetic N with it")
    run = types.SimpleNamespace(args=args)
    run.trust_on = trust_options(args)
    run.ex = optimizer_options(args)
    run.groups_on = group_options(args)
    run.cam_classes = resolve_cam_classes(getattr(args, "cam_classes", None), args.n_classes)
    if run.cam_classes is not None and not args.visualize:
        raise ValueError("--cam_classes draws class maps over the 'vis' subset: pass --visualize with it")
    run.sal = resolve_saliency(args)
    run.rank, run.world, run.local = P.dist_info()
    run.aucm = aucm_options(args, run.world)
    run.sam_on = sam_options(args, run.world)
    run.focus = focus_options(args)
    run.multiclass = multiclass_options(args)
    run.hier = hier_options(args)
    init_backbone_options(args)
    run.pretrain = pretrain_options(args, run.world)
    run.knn = knn_options(args, run.world)
    run.probe = probe_options(args, run.world)
    run.pool = resolve_pool(args)
    run.head = resolve_head(args, run.pool)
    return run


def start_process_group(args, world, local):
    """The process group comes first, before anything touches the GPU; one rank per GPU over RCCL ("nccl"), or ranks sharing a
    device over gloo when the box has fewer GPUs than ranks (tests)."""
    if world > 1:
        import torch.distributed as dist
        one_per_gpu = torch.cuda.device_count() >= world
        dist.init_process_group("nccl" if one_per_gpu else "gloo")
        args.cuda = local if one_per_gpu else 0


def open_output_dir(args, rank):
    """Phase 2: --output_dir (default results/<time>) and, on rank 0, its config.json.  Returns whether this run wrote the config: one
    kept from an earlier run (restore into its output_dir) stays whole, as that run wrote it."""
    if not args.output_dir:
        if args.restore:
            raise RuntimeError("Must specify `output_dir` argument")
        args.output_dir = os.path.join("results", time.strftime("%Y-%m-%d_%H-%M-%S", time.gmtime()))
    if rank != 0:
        return False
    os.makedirs(args.output_dir, exist_ok=True)
    cfg_path = os.path.join(args.output_dir, "config.json")
    new_cfg = not os.path.exists(cfg_path)
    if new_cfg:
        json.dump(args.__dict__, open(cfg_path, "w"), indent=4)
    return new_cfg


def add_to_config(args, key, value):
    """A resolved value goes beside the flags that asked for it, into the config.json this run created."""
    cfg_path = os.path.join(args.output_dir, "config.json")
    cfg = json.load(open(cfg_path))
    cfg[key] = value
    json.dump(cfg, open(cfg_path, "w"), indent=4)


def load_datasets(args, hier):
    """Phase 3: (training set, validation set): synthetic, or chexpert.py:64-79 over the extracted CheXpert-v1.0-small folder (uint8 to
    the GPU) with the decoded cache; under --loss hier both label tables are closed over the tree."""
    size = args.resize or 320
    if args.synthetic:
        n_valid = max(args.batch_size, args.synthetic // 5)
        train_ds = SyntheticXrays(args.mini_data or args.synthetic, size, args.n_classes, 7, args.synthetic_uncertain, args.uncertain)
        valid_ds = SyntheticXrays(n_valid, size, args.n_classes, 11)
    else:
        from .data import ChexpertCSV
        if not args.data_path:
            raise RuntimeError("pass --data_path <folder holding CheXpert-v1.0-small> or --synthetic N (no download here)")
        train_ds = ChexpertCSV(args.data_path, "train", args.resize, mini_data=args.mini_data, uncertain=args.uncertain, seed=args.seed,
                               labels=getattr(args, "labels", "competition"))
        # (under torch.distributed.run the ranks of a node share one table: --cache_decoded is then the node's budget)
        if args.cache_decoded > 0 and not train_ds.enable_decoded_cache(int(args.cache_decoded * 2 ** 30),
                                                                         node_shared=int(os.environ.get("WORLD_SIZE", "1")) > 1):
            print("decoded-image cache off: %d images of %d^2 bytes exceed --cache_decoded %.1f GB" % (len(train_ds), train_ds.crop, args.cache_decoded))
        valid_ds = ChexpertCSV(args.data_path, "valid", args.resize, mini_data=args.mini_data, labels=getattr(args, "labels", "competition"))
    if hier is not None and hier["closure"]:   # after the uncertain policy, before anything reads a table (weights, loader, evaluation)
        from .data import hierarchy_closure
        train_ds.targets = hierarchy_closure(train_ds.targets, hier["parent"])
        valid_ds.targets = hierarchy_closure(valid_ds.targets, hier["parent"])
    return train_ds, valid_ds


def resolve_label_statistics(run):
    """--pos_weight and --aucm_prior from the training table (`auto`) or the flag; what they resolved to goes into the config."""
    args = run.args
    run.pos_weight = resolve_pos_weight(args.pos_weight, run.train_ds.targets, args.n_classes)
    if run.pos_weight is not None and run.new_cfg:
        add_to_config(args, "pos_weight_resolved", run.pos_weight)
    if run.aucm is not None:
        run.aucm["prior"] = resolve_aucm_prior(args.aucm_prior, run.train_ds.targets, args.n_classes)
        if run.new_cfg:
            add_to_config(args, "aucm_prior_resolved", run.aucm["prior"])


def make_loader(args, train_ds, device):
    """Phase 4: the training loader (None without --train).  It comes BEFORE the first GPU call: its worker processes are forked from
    a process that has not initialised the GPU runtime and never touch the card (chexpert_amd/loader.py)."""
    if not args.train:
        return None
    from .loader import RingLoader
    return RingLoader(train_ds, args.batch_size, num_workers=args.num_workers, slots=4, device=device)


def start_gpu(args, device):
    if not torch.cuda.is_available():
        raise RuntimeError("chexpert_amd needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(device)
    if args.seed:
        torch.manual_seed(args.seed)
        np.random.seed(args.seed)


def build_model(run):
    """Phase 5: pooling and head as the flags and the checkpoint of --restore agree on them, the model under its optimiser, and the
    checkpoint's weights, step, optimiser state and loss state (`run.restored_loss`)."""
    args = run.args
    source = restore_source(args)
    run.pool = restore_pool(args, run.pool, source)    # the checkpoint's pooling; a --pool flag that contradicts it is refused here
    why = visualize_needs_avg(args, run.pool["kind"])
    if why:
        raise ValueError(why)
    run.head = restore_head(args, run.head, run.pool["kind"], source)  # the checkpoint's head; --head linear on a csra checkpoint is refused here
    why = visualize_needs_linear(args, run.head["kind"])
    if why:
        raise ValueError(why)
    del source
    run.model, run.optimizer, run.scheduler = make_model(args, run.device, run.pool, run.head)
    run.restored_loss = None
    if args.restore and os.path.isfile(args.restore):
        run.restored_loss = restore(args, run.model, run.optimizer, run.scheduler, run.device, run.multiclass, run.pretrain)
        adopted = run.hier is None
        run.hier = hier_for_checkpoint(run.hier, run.restored_loss, args.restore, args.train)
        if adopted and run.hier is not None and run.hier["closure"]:   # an evaluation of a --loss hier checkpoint without the flag: the
            from .data import hierarchy_closure                        # validation table as that run saw it
            run.valid_ds.targets = hierarchy_closure(run.valid_ds.targets, run.hier["parent"])
    if getattr(args, "init_backbone", None):
        keys = init_backbone(run.model, args.init_backbone, run.device)
        if run.rank == 0:
            print("--init_backbone %s: %d tensors loaded, the classifier is this run's" % (args.init_backbone, len(keys)))
    run.collapse = run.hier["parent"] if run.hier is not None else run.multiclass       # what evaluate() does to a forward's output


def summed_bce(out, t):
    return nn.BCEWithLogitsLoss(reduction="none")(out, t).sum(1).mean(0)                # chexpert.py:160


def wire_loss(run):
    """Phase 6: the loss of the fused step (FusedNet.set_loss) as the flags and a restored checkpoint's `loss_state` decide it.
    Returns (criterion, aucm_loss, aucm_opt) of the autograd route: the module that reads the storage the model holds, and under
    --loss aucm without --fused_optimizer the loss module with the optimiser of its auxiliary scalars (else None, None)."""
    args, model, pos_weight, restored_loss = run.args, run.model, run.pos_weight, run.restored_loss
    focus, hier, aucm = run.focus, run.hier, run.aucm
    criterion = summed_bce
    if pretrain_kind(run.pretrain) == "barlow":
        # as below, with lambda in the place of the temperature: --barlow_lambda has the last word, else a restored checkpoint's value
        from .loss import BarlowTwinsLoss
        lambd = lambda_of(run.pretrain, restored_loss)
        model.set_loss(kind="barlow", lambd=lambd)
        criterion = BarlowTwinsLoss(lambd)
        criterion.lambd = model.loss_lambda
        return criterion, None, None
    if run.pretrain is not None:
        # the fused step's loss and, by the same kernels, the autograd route's; one storage for the temperature: the module reads what
        # the model holds.  --temperature has the last word, else a restored checkpoint's value
        from .loss import NTXentLoss
        tau = temperature_of(run.pretrain, restored_loss)
        model.set_loss(kind="ntxent", temperature=tau)
        criterion = NTXentLoss(tau)
        criterion.temperature = model.loss_temperature
        return criterion, None, None
    if focus is not None:
        # the fused step's loss and, by the same kernel, the autograd route's; a restored checkpoint of the same kind brings its four
        # numbers (loss_focus: a schedule may have moved them), one of another kind is refused
        from .loss import AsymmetricLoss, FocalLoss
        model.set_loss(pos_weight=pos_weight, **focus)
        if restored_loss is not None:
            if restored_loss.get("kind") != focus["kind"]:
                raise ValueError("--restore: the checkpoint was trained with --loss %s, this run asks for --loss %s"
                                 % (restored_loss.get("kind"), focus["kind"]))
            model.load_loss_state(restored_loss)
        criterion = (FocalLoss if focus["kind"] == "focal" else AsymmetricLoss)(pos_weight=model.loss_pos_weight,
                                                                                **{k: v for k, v in focus.items() if k != "kind"})
        criterion.focus = model.loss_focus               # one storage: the module reads what the model holds
    elif args.train and restored_loss is not None and restored_loss.get("kind") in ("focal", "asl"):
        raise ValueError("--restore: the checkpoint was trained with --loss %s: pass it (and its flags) to go on training" % restored_loss["kind"])
    elif hier is not None:
        # the fused step's loss and, by the same kernel, the autograd route's (the table a restored checkpoint brought is this one:
        # hier_for_checkpoint); one storage for the table and the weights: the module reads what the model holds
        from .loss import HierarchicalBCE
        model.set_loss(kind="hier", parent=hier["parent"], mode=hier_mode_of(hier), pos_weight=pos_weight)
        criterion = HierarchicalBCE(hier["parent"], hier_mode_of(hier), pos_weight)
        criterion.parent, criterion.pos_weight = model.loss_parent, model.loss_pos_weight
    elif run.multiclass:
        # the fused step's loss and, by the same kernel, the autograd route's; a restored checkpoint brings its class weights
        from .loss import MultiClassUncertain
        model.set_loss(kind="multiclass")
        if restored_loss is not None:
            model.load_loss_state(restored_loss)
        criterion = MultiClassUncertain()
        criterion.class_weight = model.loss_class_weight        # one storage: the module reads what the model holds
    elif args.uncertain == "ignore" or pos_weight is not None:
        from .loss import MaskedBCE
        model.set_loss(ignore_negative=args.uncertain == "ignore", pos_weight=pos_weight)      # the fused step's loss
        criterion = MaskedBCE(model.loss_pos_weight, ignore_negative=args.uncertain == "ignore")     # the autograd route's
    aucm_loss = aucm_opt = None
    if aucm is not None:
        # the fused step's loss; a restored checkpoint brings its auxiliary scalars, the flags of this run keep the last word on
        # prior, margin and rate (set_loss on a model that holds the loss already leaves loss_aux as it is)
        if restored_loss is not None and restored_loss.get("kind") == "aucm":
            model.load_loss_state(restored_loss)
        model.set_loss(kind="aucm", **aucm)
        if args.train and not args.fused_optimizer:
            # the autograd route: the loss module's a, b, alpha under plain SGD at the auxiliary rate, then alpha >= 0 -- the update
            # of the fused step; they start from, and a checkpoint reads them back through, model.loss_aux
            from .loss import AUCMLoss
            aucm_loss = AUCMLoss(aucm["prior"], aucm["margin"]).to(run.device)
            with torch.no_grad():
                for p_, row in zip((aucm_loss.a, aucm_loss.b, aucm_loss.alpha), model.loss_aux):
                    p_.copy_(row)
            aucm_opt = torch.optim.SGD(aucm_loss.parameters(), lr=aucm["lr_aux"])
    return criterion, aucm_loss, aucm_opt


def sync_loss_aux(model, aucm_loss):
    """Autograd route: model.loss_aux (what loss_state() and a checkpoint read) follows the loss module's parameters."""
    if aucm_loss is not None:
        with torch.no_grad():
            model.loss_aux.copy_(torch.stack([aucm_loss.a, aucm_loss.b, aucm_loss.alpha]))


def averaged_weights(run):
    """The weights an evaluation during training sees: the EMA where --ema_decay keeps one (and a step has bound it)."""
    on = run.ex.get("ema_decay") is not None and run.args.train and run.model._eng().flat is not None
    return run.optimizer.ema_weights() if on else contextlib.nullcontext()


def validate(run):
    """(logits, targets, element losses) of the validation set in dataset order, every rank its shard."""
    return evaluate_sharded(run.model, run.valid_ds, run.args.batch_size, run.device, run.rank, run.world, run.clahe, run.collapse)


def run_eval(run, tag):
    args = run.args
    with averaged_weights(run):
        o, t, l = validate(run)
        knn_res, lin_res = run_probes(run)
    res = M.compute_metrics(o, t, l)
    if lin_res is not None and run.rank == 0:
        print_probe(lin_res, args.step)
        json.dump(probe_report(lin_res), open(os.path.join(args.output_dir, report_name(tag, "probe")), "w"), indent=4)
        if run.probe["save"] is not None:
            save_probe_checkpoint(run, lin_res)
    if knn_res is not None and run.rank == 0:
        print_knn(knn_res, args.step)
        json.dump(knn_res, open(os.path.join(args.output_dir, report_name(tag, "knn")), "w"), indent=4)
    if run.rank == 0:
        print("Evaluate metrics @ step %d:\nAUC:\n%s\nLoss:\n%s" % (args.step, pprint.pformat(res["aucs"]), pprint.pformat(res["loss"])))
        json.dump(res, open(os.path.join(args.output_dir, tag + ".json"), "w"), indent=4)
        write_auc_ci(args, tag, o, t, run.boot_groups)
        write_delong(args, tag, o, t, run.boot_groups)
        write_metrics_ci(args, tag, o, t, run.boot_groups)
        write_calibration(args, tag, o, t, run.boot_groups)
    return res


def jitter(x_u8, step, rank, device):
    from . import ops
    B = x_u8.shape[0]
    u = synth.uniform(step * 7919 + 13 + rank, (3, B), 0.0, 1.0)
    return ops.u8_jitter(x_u8, (0.75 + 0.5 * u[0]).to(device), (0.75 + 0.5 * u[1]).to(device),
                         (u[2] > 0.5).to(torch.int32).to(device))


def two_views(run, affine, x, idx, step, groups=None):
    """--pretrain contrastive: the uint8 minibatch, equalised once, as [x; x] with an own affine / jitter draw for each of the 2B rows,
    and the (2B, 1) ids of the contrastive loss (augment.contrastive_ids: the row's position, or its study / patient)."""
    from .augment import contrastive_ids, duplicate_views
    if run.clahe is not None:
        x = run.clahe(x)
    x = duplicate_views(x)
    if affine is not None:
        x = affine(x, step)
    if run.args.jitter:
        x = jitter(x, step, run.rank, run.device)
    return x, contrastive_ids(idx, groups).to(run.device)


def preprocess(run, affine, mix, x, t, step, idx=None):
    """The chain on the uint8 minibatch of training step `step`, every link optional.  Under --pretrain contrastive the minibatch
    becomes its two views and the target the column of ids (two_views)."""
    if run.pretrain is not None:
        return two_views(run, affine, x, idx, step, run.positive_groups)
    if run.clahe is not None:                   # deterministic preprocessing first, then the random steps
        x = run.clahe(x)
    if affine is not None:                      # geometric first, photometric second
        x = affine(x, step)
    if run.args.jitter:
        x = jitter(x, step, run.rank, run.device)
    if mix is not None:                         # per-sample transforms first, then the collated batch is mixed
        x, t = mix(x, t, step)
    return x, t


def autograd_step(run, x, t):
    """The step without --fused_optimizer: torch's optimiser (and scheduler) over the autograd route of the fused network."""
    args, optimizer, scheduler, aucm_loss, aucm_opt = run.args, run.optimizer, run.scheduler, run.aucm_loss, run.aucm_opt
    out = run.model(x)
    if run.pretrain is not None:            # (what log_line's top1 reads)
        run.last_logits = out.detach()
    if aucm_loss is not None:
        loss = aucm_loss(out, t)
        aucm_opt.zero_grad()
    else:
        loss = run.criterion(out, t)
    optimizer.zero_grad()
    loss.backward()
    optimizer.step()
    if aucm_loss is not None:
        aucm_opt.step()
        aucm_loss.clamp_()
    if scheduler and args.step >= args.lr_warmup_steps:
        scheduler.step()
    return loss


def log_line(run, loss):
    """What a --log_interval step prints, as a dict.  (loss.item() synchronises; the optimiser's figures then read the device.)"""
    ex, optimizer = run.ex, run.optimizer
    line = {"step": run.args.step, "train_loss": round(loss.item(), 5)}
    if pretrain_kind(run.pretrain) == "barlow":     # the two terms of this minibatch's loss, the off-diagonal one without its weight
        from .loss import barlow_terms
        on, off, _, _ = barlow_terms(run.last_logits, run.last_ids)
        line["on_diag"], line["off_diag"] = round(on, 5), round(off, 5)
    elif run.pretrain is not None:            # the share of this minibatch's anchors whose nearest row is a positive
        from .loss import contrastive_top1
        line["top1"] = round(contrastive_top1(run.last_logits, run.last_ids), 4)
    if ex.get("max_grad_norm") is not None or ex.get("skip_nonfinite"):
        line["grad_norm"] = round(optimizer.grad_norm(), 5)
        if optimizer.skipped_steps():
            line["skipped"] = optimizer.skipped_steps()
    if run.sam_on:
        line["sam_norm"] = round(optimizer.perturbation_norm(), 6)
    if run.trust_on:
        ratios = optimizer.adapted_ratios()
        if ratios:
            line["trust_min"], line["trust_max"] = round(min(ratios), 6), round(max(ratios), 6)
    return line


def checkpoint_dict(run, res, ema_sd):
    """The model checkpoint after the evaluation `res`, with the entries only some runs have."""
    model, hier = run.model, run.hier
    ckpt = {"global_step": run.args.step, "eval_loss": float(np.sum(list(res["loss"].values()))),
            "avg_auc": M.mean_auc(res) if run.pretrain is None else 0.0, "state_dict": model.state_dict()}
    if model.pool_kind != "avg":  # (a checkpoint without it is the average's: the keys of before)
        ckpt["pool_state"] = model.pool_state()
    if model.head_kind != "linear":
        ckpt["head_state"] = model.head_state()
    if ema_sd is not None:        # beside the live weights, which restore continues from
        ckpt["ema_state_dict"] = ema_sd
    if run.pretrain is not None:  # eval_loss is the contrastive loss; avg_auc = -eval_loss: save_checkpoint keeps the lowest-loss files
        ckpt["pretrain"], ckpt["avg_auc"] = pretrain_kind(run.pretrain), -ckpt["eval_loss"]
        ckpt["loss_state"] = dict(model.loss_state(), positive=run.pretrain["positive"])
    elif run.aucm is not None:    # the auxiliary scalars are trained state: restore continues from them
        sync_loss_aux(model, run.aucm_loss)
        ckpt["loss_state"] = model.loss_state()
    elif run.focus is not None or run.multiclass or hier is not None:      # the loss's numbers: restore checks the kind and puts them back
        ckpt["loss_state"] = model.loss_state()
        if hier is not None:          # how the label tables were made: an evaluation without the flags does the same
            ckpt["loss_state"]["closure"] = hier["closure"]
    return ckpt


EVAL_VIEW_STEP = 1 << 30          # the "step" the validation views of --pretrain contrastive are drawn from: minibatch b uses this + b


@torch.no_grad()
def contrastive_eval(run):
    """--pretrain contrastive at an evaluation: the contrastive loss (the mean over the anchors of the whole set, each contrasted within
    its minibatch of two views) and the top-1 share over the validation set, in eval mode, from views drawn from a fixed seed.
    Printed, written to pretrain_eval_step_<n>.json, and returned in the shape checkpoint_dict reads ({"loss": {...}})."""
    if pretrain_kind(run.pretrain) == "barlow":
        return barlow_eval(run)
    from .loss import contrastive_top1
    args, model = run.args, run.model
    model.eval()
    codes = positive_codes(run.pretrain["positive"], run.valid_ds)          # (`batches` yields positions)
    total, hits, anchors = 0.0, 0, 0
    for b, (x, _, idx) in enumerate(batches(run.valid_ds, list(range(len(run.valid_ds))), args.batch_size, False)):
        x, ids = two_views(run, run.affine, x.to(run.device), idx, EVAL_VIEW_STEP + b, codes)
        out = model(x)
        le = run.criterion.elementwise(out, ids)
        h, a = contrastive_top1(out, ids, return_counts=True)
        total, hits, anchors = total + float(le.sum().item()), hits + h, anchors + a
    res = {"pretrain": "contrastive", "step": args.step, "loss": {"contrastive": total / max(anchors, 1)},
           "top1": hits / max(anchors, 1), "anchors": anchors, "temperature": float(model.loss_temperature.item()),
           "positive": run.pretrain["positive"]}
    knn_res, lin_res = run_probes(run)
    model.eval()
    if knn_res is not None:
        res["knn"] = knn_res
        if run.rank == 0:
            print_knn(knn_res, args.step)
    if lin_res is not None:
        res["linear_probe"] = probe_report(lin_res)
        if run.rank == 0:
            print_probe(lin_res, args.step)
    if run.rank == 0:
        print("Evaluate contrastive pretraining @ step %d: loss %.5f, top1 %.4f over %d anchors" % (args.step, res["loss"]["contrastive"],
                                                                                                 res["top1"], anchors))
        json.dump(res, open(os.path.join(args.output_dir, "pretrain_eval_step_%d.json" % args.step), "w"), indent=4)
    return res


@torch.no_grad()
def barlow_eval(run):
    """--pretrain barlow at an evaluation: the Barlow Twins loss and its terms over the validation set, in eval mode, from views drawn
    from a fixed seed -- each minibatch of two views is normalised and correlated within itself, and the figures are the means over
    the minibatches weighted by their pairs m (a last minibatch of one image has no pair statistics and weighs nothing).  Printed,
    written to pretrain_eval_step_<n>.json, and returned in the shape checkpoint_dict reads ({"loss": {...}})."""
    from .loss import barlow_terms
    args, model = run.args, run.model
    model.eval()
    lambd = float(model.loss_lambda.item())
    sums, pairs = np.zeros(4), 0
    for b, (x, _, idx) in enumerate(batches(run.valid_ds, list(range(len(run.valid_ds))), args.batch_size, False)):
        x, ids = two_views(run, run.affine, x.to(run.device), idx, EVAL_VIEW_STEP + b, None)
        out = model(x)
        on, off, diag, m = barlow_terms(out, ids)
        if m >= 2:
            sums += m * np.array([float(run.criterion(out, ids).item()), on, off, diag])
            pairs += m
    mean = sums / max(pairs, 1)
    res = {"pretrain": "barlow", "step": args.step, "loss": {"barlow": float(mean[0])}, "on_diag": float(mean[1]), "off_diag": float(mean[2]),
           "mean_diag": float(mean[3]), "pairs": int(pairs), "lambda": lambd}
    knn_res, lin_res = run_probes(run)
    model.eval()
    if knn_res is not None:
        res["knn"] = knn_res
        if run.rank == 0:
            print_knn(knn_res, args.step)
    if lin_res is not None:
        res["linear_probe"] = probe_report(lin_res)
        if run.rank == 0:
            print_probe(lin_res, args.step)
    if run.rank == 0:
        print("Evaluate Barlow Twins pretraining @ step %d: loss %.5f (on %.5f, off %.5f, mean diagonal %.4f) over %d pairs"
              % (args.step, res["loss"]["barlow"], res["on_diag"], res["off_diag"], res["mean_diag"], pairs))
        json.dump(res, open(os.path.join(args.output_dir, "pretrain_eval_step_%d.json" % args.step), "w"), indent=4)
    return res


def evaluate_and_checkpoint(run, graphed):
    """An --eval_interval step: the validation metrics under the averaged weights and, on rank 0, the checkpoint files."""
    model, optimizer, scheduler = run.model, run.optimizer, run.scheduler
    ema_sd = None
    with averaged_weights(run):
        res = M.compute_metrics(*validate(run)) if run.pretrain is None else contrastive_eval(run)
        if run.ex.get("ema_decay") is not None and run.rank == 0:
            ema_sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    if run.rank == 0:
        if graphed:
            optimizer.sync_from_device()
        sched_state = scheduler.state_dict() if scheduler is not None and scheduler != "fused" else None
        save_checkpoint(checkpoint_dict(run, res, ema_sd), optimizer.state_dict(), sched_state, run.args)
    model.train()


def train(run):
    """Phase 7: the epoch loop.  Every fused step is the optimiser's train_step (optim._Flat.train_step, optim.FusedSAM.train_step):
    replayed from the graph captured on the first full minibatch, launched one by one on the device-resident state for a partial
    minibatch of a graphed run, or launched with the host's learning rate and scheduler."""
    args, model, optimizer, scheduler, rank, world, device = run.args, run.model, run.optimizer, run.scheduler, run.rank, run.world, run.device
    affine = run.affine = make_affine(args, rank, device)
    mix = make_mix(args, rank, device)
    run.positive_groups = None
    if run.pretrain is not None:                  # --positive study | patient: the index of every training row's study / patient,
        run.positive_groups = positive_codes(run.pretrain["positive"], run.train_ds, by_label=True)      # by the loader's row label
    fused = args.fused_optimizer
    gstep = None
    full = args.batch_size * (2 if run.pretrain is not None else 1)     # rows of a full minibatch as the step sees it
    if world > 1:            # replicas start identical (parameters, buffers) and average their gradients inside backward from
        model._eng().bind(device)                 # the first step on: bind the flat buffers now, before any optimiser state exists
        P.broadcast_module_state(model)
        model._eng().enable_data_parallel()
    for epoch in range(args.n_epochs):
        model.train()
        idx = P.shard_indices(len(run.train_ds), rank, world, seed=args.seed or 1, epoch=epoch)
        if not idx:
            raise RuntimeError("the training set (%d images over %d ranks) yields no minibatch" % (len(run.train_ds), world))
        t_epoch = time.perf_counter()
        # every image is seen each epoch, as with the reference's DataLoader (drop_last=False, chexpert.py:76): the last,
        # partial minibatch runs as an eager step (the hipGraph is captured on the full batch's shapes)
        for x, t, rows in run.train_loader.batches(idx, drop_last=False):
            args.step += 1
            x, t = preprocess(run, affine, mix, x, t, args.step, rows)
            run.last_ids = t
            if args.graph and fused and (gstep is not None or x.shape[0] == full):
                if gstep is None:                       # captured on the first full minibatch's shapes
                    # (data-parallel: graph segments cut at the gradient buckets, the all-reduces enqueued between them)
                    from .graph import GraphedTrainStep, SegmentedTrainStep
                    gstep = (GraphedTrainStep if world == 1 else SegmentedTrainStep)(model, optimizer, x, t,
                                                                                      warmup_steps=int(args.lr_warmup_steps))
                if x.shape[0] == full:
                    loss, run.last_logits = gstep.replay(x, t)
                else:                                   # same device-resident optimiser / scheduler state, launched one by one
                    loss, run.last_logits = optimizer.train_step(model, x, t, dev=True)
            elif fused:
                loss, run.last_logits = optimizer.train_step(model, x, t)         # chexpert.py:159-163 as one fused schedule
                if scheduler == "fused" and args.step >= args.lr_warmup_steps:
                    optimizer.scheduler_step()
            else:
                loss = autograd_step(run, x, t)
            if run.groups_on.get("freeze_steps", 0) > 0 and args.step == run.groups_on["freeze_steps"]:
                thaw_backbone(optimizer)                # every rank alike: the table is the same on all of them, no collective
            if args.step % args.log_interval == 0 and rank == 0:
                print(json.dumps(log_line(run, loss)), flush=True)
            if args.step % args.eval_interval == 0:
                evaluate_and_checkpoint(run, gstep is not None)
        sync_loss_aux(model, run.aucm_loss)      # (also current when no checkpoint followed the last step)
        torch.cuda.synchronize()
        if rank == 0:        # input pipeline + step, end to end (the figure to hold against bench.py's device-resident rate)
            print(json.dumps({"epoch": epoch, "images_per_sec": round(len(idx) * world / (time.perf_counter() - t_epoch), 1),
                              "loader_workers": args.num_workers,
                              "decoded_cache_fill": round(run.train_ds.cache_fill(), 3) if hasattr(run.train_ds, "cache_fill") else None}), flush=True)
        if run.pretrain is None:
            run_eval(run, "eval_results_step_%d" % args.step)
        else:
            with averaged_weights(run):
                contrastive_eval(run)


def evaluate_ensemble(run):
    """chexpert.py:214-240: the mean of the logits of every checkpoint of the folder --restore names."""
    args, model, boot_groups = run.args, run.model, run.boot_groups
    assert args.restore and os.path.isdir(args.restore), "Restore argument must be directory with saved checkpoints"
    outs, losses, members = [], [], []
    for c in checkpoint_files(args.restore):
        ck = torch.load(os.path.join(args.restore, c), map_location=run.device)
        check_checkpoint_pretrain(ck, None, c)
        check_checkpoint_head(ck, run.multiclass, c)
        check_member_hier(run.hier, ck, c)
        check_checkpoint_pool(ck, model, c)
        check_checkpoint_head_kind(ck, model, c)
        model.load_state_dict(model_weights(ck, args, c))
        o, tg, l = validate(run)
        outs.append(o)
        losses.append(l)
        members.append(c)
    mean_out = torch.stack(outs, 2).mean(2)                                                      # mean of logits, chexpert.py:233
    res = M.compute_metrics(mean_out, tg, torch.stack(losses, 2).mean(2))
    if run.rank == 0:
        json.dump(res, open(os.path.join(args.output_dir, "eval_results_ensemble.json"), "w"), indent=4)
        print("AUC:\n", pprint.pformat(res["aucs"]))
        write_auc_ci(args, "eval_results_ensemble", mean_out, tg, boot_groups)
        write_delong(args, "eval_results_ensemble", mean_out, tg, boot_groups, members=dict(zip(members, outs)))
        write_metrics_ci(args, "eval_results_ensemble", mean_out, tg, boot_groups)
        write_calibration(args, "eval_results_ensemble", mean_out, tg, boot_groups)


def visualize(run):
    """chexpert.py:556-563: Grad-CAM grids over the 'vis' subset (three examples per finding category), and for the
    attention-augmented models the attention-map grids of the stored softmax weights; the class maps of --cam_classes and the
    pixel attributions of --saliency."""
    from . import vis
    from .gradcam import class_cam, grad_cam
    args, model, device, valid_ds, clahe, hier, cam_classes, sal = (run.args, run.model, run.device, run.valid_ds, run.clahe, run.hier,
                                                                    run.cam_classes, run.sal)
    names = class_names(args.n_classes, getattr(args, "labels", "competition"))
    to_binary = collapse_of(hier["parent"]) if hier is not None else None    # the figures' scores are unconditional probabilities;
    groups = vis.select_vis_subset(valid_ds.targets, names)
    flat = sorted({i for g in groups[1] for i in g})
    pos = {i: k for k, i in enumerate(flat)}
    imgs, labels, scores, masks, class_maps, sal_maps = [], [], [], [], [], []
    model.eval()
    attn_layers = [m for m in model.modules() if type(m).__name__ == "AAConv2d"]
    csra = model.head_kind == "csra"       # (its figures: the score and attention maps of --cam_classes, and the saliency maps)
    pcam = model.head_kind == "pcam"       # (its figures: the probability maps of --cam_classes, and the saliency maps)
    avg_pool = model.pool_kind == "avg" and not csra and not pcam
    csra_maps, pcam_up = [], []
    for x, tg, idx in batches(valid_ds, flat, args.batch_size, False):
        xd = x.to(device)
        if clahe is not None:                # the figures show what the network saw
            xd = clahe(xd)
            x = xd.cpu()
        with torch.no_grad():              # the maps below stay those of the conditional logits: evidence for a finding GIVEN its parent
            scores.append((model(xd) if to_binary is None else to_binary(model(xd))).float().cpu())
        if avg_pool:                         # (another pooling: the saliency maps are the figures, visualize_needs_avg)
            masks.append(grad_cam(model, xd).float().cpu())
        if cam_classes is not None and (csra or pcam):
            from .heads import class_maps as head_maps
            sc_map, at_map, _ = head_maps(model, xd)
            csra_maps.append(torch.stack([sc_map[:, cam_classes], at_map[:, cam_classes]], 1).cpu())
            if pcam:                        # the overlays: P of the requested classes, scaled per map and up-sampled on the GPU
                from . import ops
                pm = sc_map[:, cam_classes].contiguous()
                up = torch.empty(pm.shape[0] * pm.shape[1], 1, xd.shape[2], xd.shape[3], dtype=torch.float32, device=device)
                ops.cam_norm_upsample(pm.view(up.shape[0], -1), up, pm.shape[2], pm.shape[3])
                pcam_up.append(up.view(pm.shape[0], pm.shape[1], xd.shape[2], xd.shape[3]).half().cpu())
        elif cam_classes is not None:       # the raw low-resolution relu(M): up-sampled maps of 14 classes would be hundreds of MB
            class_maps.append(class_cam(model, xd, cam_classes, normalize=False, upsample=False)[0].cpu())
        if sal is not None:                 # float interface: whitened, three identical channels (as the attention figures below)
            xf = ((xd.float().div(255.0) - vis.MEAN) / vis.STD).expand(-1, 3, -1, -1) if xd.dtype == torch.uint8 else xd.float()
            sal_maps.append(saliency_maps(model, xf.contiguous(), sal).cpu())
        imgs.append(x.float().div(255.0)[:, 0] if x.dtype == torch.uint8 else (x.float()[:, 0] * vis.STD + vis.MEAN))
        labels.append(tg)
        if attn_layers:
            xn = (x.float().div(255.0) - vis.MEAN) / vis.STD if x.dtype == torch.uint8 else x.float()
            for k in range(len(x)):
                vis.vis_attn(xn, ["synthetic/%d" % int(i) for i in idx], idx, attn_layers, args.output_dir, k)
    imgs, labels, scores = torch.cat(imgs), torch.cat(labels), torch.cat(scores)
    groups = (groups[0], [[pos[i] for i in g] for g in groups[1]])
    if avg_pool:
        cam = masks = torch.cat(masks)
        files = vis.visualize(imgs.numpy(), labels.numpy(), scores.numpy(), masks[:, 0].numpy(), ["synthetic/%d" % i for i in flat], names,
                              groups, args.output_dir, getattr(args, "step", 0))
        np.save(os.path.join(args.output_dir, "vis", "grad_cam.npy"), cam.numpy())
        print("grad-cam maps:", tuple(cam.shape), "figures:", len(files))
    if cam_classes is not None and pcam:
        csra_maps = torch.cat(csra_maps)
        files = vis.visualize_classes(imgs.numpy(), labels.numpy(), scores.numpy(), torch.cat(pcam_up).float().numpy(),
                                      ["synthetic/%d" % i for i in flat], names, cam_classes, args.output_dir, getattr(args, "step", 0),
                                      prefix="pcam")
        np.save(os.path.join(args.output_dir, "vis", "pcam_maps_lowres.npy"), csra_maps.numpy())
        print("pcam probability / weight maps:", tuple(csra_maps.shape), "figures:", len(files))
    elif cam_classes is not None and csra:
        csra_maps = torch.cat(csra_maps)
        os.makedirs(os.path.join(args.output_dir, "vis"), exist_ok=True)
        np.save(os.path.join(args.output_dir, "vis", "csra_maps_lowres.npy"), csra_maps.numpy())
        print("csra score / attention maps:", tuple(csra_maps.shape))
    elif cam_classes is not None:
        class_maps = torch.cat(class_maps)
        files = vis.visualize_classes(imgs.numpy(), labels.numpy(), scores.numpy(), class_maps.numpy(), ["synthetic/%d" % i for i in flat],
                                      names, cam_classes, args.output_dir, getattr(args, "step", 0))
        np.save(os.path.join(args.output_dir, "vis", "class_cam_lowres.npy"), class_maps.numpy())
        print("class maps:", tuple(class_maps.shape), "figures:", len(files))
    if sal is not None:
        sal_maps = torch.cat(sal_maps)
        files = vis.visualize_saliency(imgs.numpy(), labels.numpy(), scores.numpy(), sal_maps.numpy(), ["synthetic/%d" % i for i in flat],
                                       names, sal["classes"], sal["method"], args.output_dir, getattr(args, "step", 0),
                                       signed=sal["method"] == "ig")
        # fp16 on disk: every map divided by its largest magnitude (gradients of a logit per pixel are far below fp16's range)
        scale = sal_maps.abs().amax((2, 3))
        np.save(os.path.join(args.output_dir, "vis", "saliency_%s.npy" % sal["method"]),
                (sal_maps / scale.clamp_min(1e-30)[:, :, None, None]).numpy().astype(np.float16))
        np.save(os.path.join(args.output_dir, "vis", "saliency_%s_scale.npy" % sal["method"]), scale.numpy())
        print("saliency (%s) maps:" % sal["method"], tuple(sal_maps.shape), "figures:", len(files))


def plot_all_roc(args):
    files = [f for f in os.listdir(args.output_dir) if f.startswith("eval_results") and f.endswith(".json")]
    if not files:
        raise RuntimeError("No `eval_results` files found in `%s` to plot results from." % args.output_dir)
    for f in files:
        plot_roc(json.load(open(os.path.join(args.output_dir, f))), args, "roc_pr_" + f.split(".")[0])


def main(argv=None):
    """The phases of the module docstring, in order; returns the model."""
    run = check_flags(argv)
    args = run.args
    start_process_group(args, run.world, run.local)
    run.new_cfg = open_output_dir(args, run.rank)
    run.device = torch.device("cuda:%d" % (args.cuda or 0))
    run.train_ds, run.valid_ds = load_datasets(args, run.hier)
    resolve_label_statistics(run)
    run.train_loader = make_loader(args, run.train_ds, run.device)
    try:            # the loader's worker processes end with training, however it ends
        start_gpu(args, run.device)
        build_model(run)
        run.criterion, run.aucm_loss, run.aucm_opt = wire_loss(run)
        if run.rank == 0:
            print("Loaded %s (number of parameters: %s; weights trained to step %d)" % (
                run.model._get_name(), format(sum(p.numel() for p in run.model.parameters()), ","), args.step))
        run.clahe = make_clahe(args)
        run.boot_groups = None
        if getattr(args, "bootstrap", 0) > 0 or getattr(args, "delong", False):
            run.boot_groups = bootstrap_groups(args, run.valid_ds)
        if args.train:
            train(run)
    finally:
        if run.train_loader is not None:
            run.train_loader.close()
    if args.evaluate_single_model:
        run_eval(run, "eval_results_step_%d" % args.step)
    if args.evaluate_ensemble:
        evaluate_ensemble(run)
    if args.visualize and run.rank == 0:
        visualize(run)
    if args.plot_roc and run.rank == 0:
        plot_all_roc(args)
    if run.world > 1:
        import torch.distributed as dist
        dist.barrier()
        dist.destroy_process_group()
    return run.model


if __name__ == "__main__":
    main()
