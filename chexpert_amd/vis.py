"""Visualisation outputs of the reference's `--visualize` mode, host side (matplotlib, Agg): the Grad-CAM grids of
chexpert.py:305-361 (`visualize`, `visualize_one`) and the attention-map grids of chexpert.py:363-397 (`vis_attn`), with the
subset selection of dataset.py:50-68 (mode 'vis').  The maps themselves come from the HIP path (gradcam.grad_cam,
AAConv2d.weights); this module only arranges them into the same figures and file names.
"""
import os

import numpy as np
import torch

MEAN, STD = 0.5330, 0.0349        # chexpert.py:71 (Normalize) -- undone before display


def select_vis_subset(targets, attr_names, per_group=3):
    """dataset.py:50-68: up to three examples with exactly one finding for every attribute, then three with no finding, three with
    two findings and three with more; returns (group names, list of index lists)."""
    t = torch.as_tensor(targets).float()
    total = t.sum(1)
    groups = []
    for a in range(len(attr_names)):
        groups.append(torch.nonzero((t[:, a] == 1) & (total == 1)).flatten()[:per_group].tolist())
    groups.append(torch.nonzero(total == 0).flatten()[:per_group].tolist())
    groups.append(torch.nonzero(total == 2).flatten()[:per_group].tolist())
    groups.append(torch.nonzero(total > 2).flatten()[:per_group].tolist())
    return list(attr_names) + ["No findings", "2 conditions", "Multiple conditions"], groups


def _plt():
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    return plt


def _row(plt, axs, img, mask, label, prob, ident, attr_names):
    """One example: [ground truth / predicted probability table | image | Grad-CAM over the image] (chexpert.py:339-361)."""
    order = np.argsort(-prob)
    lab, pr = label[order], prob[order]
    names = [attr_names[i] for i in order]
    cells = np.stack([lab, pr.round(3)], 1)
    axs[0].set_title(str(ident))
    axs[0].table(cellText=cells, rowLabels=names, colLabels=["Ground truth", "Pred. prob"], rowColours=plt.cm.Greens(0.5 * lab),
                 cellColours=plt.cm.Greens(0.5 * cells), cellLoc="center", loc="center")
    axs[0].axis("tight")
    axs[1].set_title("Original image", fontsize=10)
    axs[1].imshow(img, cmap="gray")
    axs[2].set_title("Top class activation \n%s: %.4f" % (names[0], pr[0]), fontsize=10)
    axs[2].imshow(img, cmap="gray")
    axs[2].imshow(mask, cmap="jet", alpha=0.5)
    for ax in axs:
        ax.axis("off")


def visualize(imgs, labels, logits, masks, idents, attr_names, groups, out_dir, step):
    """imgs (N,H,W) in [0,1], labels (N,C), logits (N,C), masks (N,H,W) Grad-CAM in [0,1]; groups = (names, index lists into the N
    examples).  One figure of up to 3 rows x 3 columns per group, saved as vis/vis_<group>_step_<step>.png (chexpert.py:326-337)."""
    plt = _plt()
    os.makedirs(os.path.join(out_dir, "vis"), exist_ok=True)
    probs = 1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float64)))
    written = []
    for name, idxs in zip(*groups):
        fig, axs = plt.subplots(3, 3, figsize=(4 * imgs.shape[1] / 100, 3.3 * imgs.shape[2] / 100), dpi=100, frameon=False)
        fig.suptitle(name)
        for r in range(3):
            if r < len(idxs):
                i = idxs[r]
                _row(plt, axs[r], imgs[i], masks[i], np.asarray(labels[i], dtype=np.float64), probs[i], idents[i], attr_names)
            else:
                for ax in axs[r]:
                    ax.axis("off")
        path = os.path.join(out_dir, "vis", "vis_%s_step_%d.png" % (name.replace(" ", "_"), step))
        plt.savefig(path, dpi=100)
        plt.close(fig)
        written.append(path)
    return written


def vis_attn(x, idents, idxs, attn_layers, out_dir, batch_element=0, window=30):
    """chexpert.py:363-397: for every attention layer a grid with one column per probed pixel (the corners of the centre third of the
    image) and one row per head below a row of images with the probed window marked; the maps are the layer's softmax weights
    (AAConv2d.weights, (B, nh, HW, HW)) averaged over the window.  x: (B,C,H,W) normalised images on the CPU."""
    plt = _plt()
    os.makedirs(os.path.join(out_dir, "vis"), exist_ok=True)
    H, W = x.shape[2:]
    corners = lambda h, w: [(h // 3, w // 3), (h // 3, int(2 * w / 3)), (int(2 * h / 3), w // 3), (int(2 * h / 3), int(2 * w / 3))]
    written = []
    for j, layer in enumerate(attn_layers):
        nh = layer.nh
        attn = layer.weights.detach()[batch_element].float().cpu()
        side = int(round(float(np.sqrt(attn.shape[-1]))))
        attn = attn.reshape(nh, side, side, side, side)
        ws = max(1, int(window * side / H))
        fig, axs = plt.subplots(nh + 1, 4, figsize=(3, 3 / 4 * (1 + nh)), frameon=False)
        fig.suptitle(str(idents[batch_element]), fontsize=8)
        base = (x[batch_element].detach().float().cpu() * STD + MEAN).clamp(0, 1)
        if base.shape[0] == 1:
            base = base.expand(3, -1, -1)
        for ax, (ph, pw) in zip(axs[0], corners(H, W)):
            im = base.clone()
            im[:, max(ph - window, 0):ph + window, max(pw - window, 0):pw + window] = torch.tensor([1.0, 215 / 255, 0.0]).view(3, 1, 1)
            ax.imshow(im.permute(1, 2, 0).numpy())
            ax.axis("off")
        for i, (ph, pw) in enumerate(corners(side, side)):
            for h in range(nh):
                patch = attn[h, max(ph - ws, 0):ph + ws, max(pw - ws, 0):pw + ws]
                axs[h + 1, i].imshow(patch.mean((0, 1)).numpy())
                axs[h + 1, i].axis("off")
        path = os.path.join(out_dir, "vis", "attn_image_idx_%d_%d_layer_%d.png" % (int(idxs[batch_element]), batch_element, j))
        fig.subplots_adjust(0, 0, 1, 0.95, 0.05, 0.05)
        plt.savefig(path)
        plt.close(fig)
        written.append(path)
    return written


def visualize_classes(imgs, labels, logits, cams, idents, attr_names, classes, out_dir, step, prefix="classcam"):
    """Per-finding localisation figures (gradcam.class_cam): imgs (N,H,W) in [0,1], labels (N,C), logits (N,C), cams (N,K,h,w) the maps
    of the K classes `classes` (indices into attr_names) at any resolution -- each is scaled to its own range and stretched over
    the image for display.  One figure per image, vis/classcam_<ident>_step_<step>.png: the radiograph, then one overlay per class
    titled with the class name, its label and its sigmoid probability (plotting conventions of `_row`).  `prefix` replaces
    `classcam` in the file name (the pcam head's probability maps: "pcam")."""
    plt = _plt()
    os.makedirs(os.path.join(out_dir, "vis"), exist_ok=True)
    probs = 1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float64)))
    cams = np.asarray(cams, dtype=np.float64)
    K = len(classes)
    assert cams.ndim == 4 and cams.shape[1] == K, "cams: (N, K, h, w) with one map per requested class"
    H, W = imgs.shape[1], imgs.shape[2]
    written = []
    for i in range(len(imgs)):
        fig, axs = plt.subplots(1, K + 1, figsize=((K + 1) * max(W, 128) / 100, 1.3 * max(H, 128) / 100), dpi=100, frameon=False, squeeze=False)
        axs = axs[0]
        axs[0].set_title("%s\nOriginal image" % idents[i], fontsize=10)
        axs[0].imshow(imgs[i], cmap="gray")
        for k, c in enumerate(classes):
            m = cams[i, k]
            m = (m - m.min()) / (m.max() - m.min() + 1e-5)
            axs[k + 1].set_title("%s\nlabel %g, prob. %.4f" % (attr_names[c], float(labels[i][c]), probs[i][c]), fontsize=10)
            axs[k + 1].imshow(imgs[i], cmap="gray")
            axs[k + 1].imshow(m, cmap="jet", alpha=0.5, extent=(-0.5, W - 0.5, H - 0.5, -0.5), interpolation="bilinear")
        for ax in axs:
            ax.axis("off")
        path = os.path.join(out_dir, "vis", "%s_%s_step_%d.png" % (prefix, str(idents[i]).replace("/", "_").replace(" ", "_"), step))
        plt.savefig(path, dpi=100)
        plt.close(fig)
        written.append(path)
    return written


def visualize_saliency(imgs, labels, logits, maps, idents, attr_names, classes, method, out_dir, step, signed=False):
    """Pixel attribution figures (chexpert_amd.saliency): imgs (N,H,W) in [0,1], labels (N,C), logits (N,C), maps (N,K,H,W) the
    full-resolution maps of the K classes `classes` (indices into attr_names).  One figure per image,
    vis/saliency_<method>_<ident>_step_<step>.png: the radiograph, then one overlay per class titled as in `visualize_classes`.
    The display scaling happens here, on the host, per map: its 99.5th percentile of |map| is the end of the colour range (a single
    hot pixel does not flatten the rest); signed maps (integrated gradients) get a symmetric diverging colour map around zero,
    unsigned ones a sequential one from zero."""
    plt = _plt()
    os.makedirs(os.path.join(out_dir, "vis"), exist_ok=True)
    probs = 1.0 / (1.0 + np.exp(-np.asarray(logits, dtype=np.float64)))
    maps = np.asarray(maps, dtype=np.float64)
    K = len(classes)
    assert maps.ndim == 4 and maps.shape[1] == K and maps.shape[2:] == imgs.shape[1:], "maps: (N, K, H, W), one map per requested class"
    H, W = imgs.shape[1], imgs.shape[2]
    written = []
    for i in range(len(imgs)):
        fig, axs = plt.subplots(1, K + 1, figsize=((K + 1) * max(W, 128) / 100, 1.3 * max(H, 128) / 100), dpi=100, frameon=False, squeeze=False)
        axs = axs[0]
        axs[0].set_title("%s\nOriginal image" % idents[i], fontsize=10)
        axs[0].imshow(imgs[i], cmap="gray")
        for k, c in enumerate(classes):
            m = maps[i, k]
            top = float(np.percentile(np.abs(m), 99.5))
            top = top if top > 0 else (float(np.abs(m).max()) or 1.0)
            axs[k + 1].set_title("%s\nlabel %g, prob. %.4f" % (attr_names[c], float(labels[i][c]), probs[i][c]), fontsize=10)
            axs[k + 1].imshow(imgs[i], cmap="gray")
            if signed:
                axs[k + 1].imshow(m, cmap="seismic", vmin=-top, vmax=top, alpha=0.6)
            else:
                axs[k + 1].imshow(np.abs(m), cmap="inferno", vmin=0.0, vmax=top, alpha=0.6)
        for ax in axs:
            ax.axis("off")
        path = os.path.join(out_dir, "vis", "saliency_%s_%s_step_%d.png" % (method, str(idents[i]).replace("/", "_").replace(" ", "_"), step))
        plt.savefig(path, dpi=100)
        plt.close(fig)
        written.append(path)
    return written


def reliability_diagram(reliability, attr_names, out_path, after=None):
    """Reliability diagram of calibration.calibration_metrics' "reliability" entry: one panel per class with the diagonal, the curve
    fraction positive against mean confidence over the non-empty bins (`reliability`: before the map; `after`, optional: with it), and
    under it the bin weights of `reliability` as a bar strip at the bins' mean confidence.  Class keys may be ints or, after a json
    round trip, strings.  Writes out_path (png) and returns it."""
    plt = _plt()

    def curve(rel, c):
        get = lambda d: np.asarray(d[c] if c in d else d[str(c)], dtype=np.float64)
        return get(rel["mean_conf"]), get(rel["frac_pos"]), get(rel["weight"])
    C = len(reliability["weight"])
    fig, axs = plt.subplots(2, max(C, 1), figsize=(3.0 * max(C, 1), 3.8), dpi=100, squeeze=False, sharex=True,
                            gridspec_kw={"height_ratios": [4, 1]})
    for c in range(C):
        top, strip = axs[0][c], axs[1][c]
        top.plot([0, 1], [0, 1], color="0.6", linestyle="--", linewidth=1)
        x, y, w = curve(reliability, c)
        ok = w > 0
        top.plot(x[ok], y[ok], marker="o", markersize=3, linewidth=1, label="before" if after is not None else None)
        if after is not None:
            xa, ya, wa = curve(after, c)
            top.plot(xa[wa > 0], ya[wa > 0], marker="s", markersize=3, linewidth=1, label="after")
            top.legend(fontsize=7, loc="upper left")
        top.set_xlim(0, 1)
        top.set_ylim(0, 1)
        top.set_title(attr_names[c] if c < len(attr_names) else "class %d" % c, fontsize=9)
        if c == 0:
            top.set_ylabel("fraction positive", fontsize=8)
            strip.set_ylabel("weight", fontsize=8)
        strip.bar(x[ok], w[ok], width=1.0 / max(int(reliability["bins"]), 1) * 0.8, color="0.4")
        strip.set_xlabel("mean confidence", fontsize=8)
        for ax in (top, strip):
            ax.tick_params(labelsize=7)
    fig.tight_layout()
    plt.savefig(out_path, dpi=100)
    plt.close(fig)
    return out_path
