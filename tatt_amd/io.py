"""Checkpoint files and the evaluation metrics loop in the reference's formats.

* `save_checkpoint` writes what `TextBase.save_checkpoint` writes (reference interfaces/base.py:621-672): one file per generator
  with the dict {'state_dict_G', 'info', 'best_history_res', 'best_model_info', 'param_num', 'converge'} as
  `model_best_<prefix>_<i>.pth` / `checkpoint.pth`, the recognisers' state_dicts beside them.
* `load_generator` mirrors the resume branch of `TextBase.generator_init` (reference interfaces/base.py:398-443): a file or a
  directory, with or without the 'state_dict_G' wrapper, `module.`-prefixed keys of DataParallel checkpoints accepted in both
  directions.
* `evaluate` is the metric part of the reference's eval loop (interfaces/super_resolution.py:1409-1420,1454-1455): PSNR and SSIM
  of the SR images against HR on the first three channels, averaged over batches -- computed by the HIP kernels -- and, given a
  CRNN recogniser and the label strings, the recognition accuracies of the SR / LR / HR images (:1374-1396,1527-1558,1662-1664;
  greedy CTC decoding = utils/metrics.py:71-92, string filter = utils/util.py:12-32).
* `collate_labels` / `collate_batch` produce the batch tuple the reference's loaders hand to the loop
  (dataset/dataset.py:1966-2077, alignCollate_realWTLAMask.__call__): images stacked, labels stretched to 26 steps and one-hot
  encoded as the (B, 37, 1, 26) text prior, the per-character class list and the blank flags.
* `resize_normalize` / `collate_pil_batch` are the image half of that collate (`resizeNormalize`, dataset/dataset.py:1266-1319; the
  transform calls of :1987-2003): PIL bicubic resize to the HR / LR size, uint8 -> float / 255 in CHW, and the binarised mask channel
  (gray < mean -> 1) as the fourth plane -- the (B, 4, H, W) tensors the generator reads.  Pinned by `tests/golden/collate.npz`,
  generated from the reference's own collate (tools/gen_golden_collate.py).
* `DeviceCollator` is `collate_pil_batch` with the image stacks built on the GPU: one packing pass over raw bytes, one copy, one HIP
  launch (csrc/collate.hip) whose result is bit for bit the host path's; `collate_plan` is its host half.
* `export_pil_batch` is the way back, the reference's per-image export of an image tensor (interfaces/super_resolution.py:1572-1591:
  `.cpu().numpy() * 255`, clip, `astype(np.uint8)`, resize; interfaces/base.py:565-618 for the `save_image` rounding) on the host;
  `DeviceExporter` is the same with the pixels made on the GPU: one HIP launch (csrc/export.hip), one copy back of uint8, byte for byte the
  host path's; `export_plan` / `panel_layout` are its host half.
* `line_plan` / `line_windows_host` / `blend_windows_host` / `super_resolve_lines_host` (tatt_amd/lines.py, re-exported here) take a
  text line of any width through a generator that knows one LR size: windows of the line at its own aspect ratio, merged back with tent
  weights; `DeviceCollator.windows` and `DeviceExporter.lines` are the same on the GPU (csrc/lines.hip), bit for bit.
* `quad_check` / `quad_matrices` / `warp_u8_host` / `quad_compose_host` / `super_resolve_quads_host` (tatt_amd/quads.py, re-exported here)
  take a detector's QUADRILATERALS instead of boxes: every quad rectified into an upright crop, the finished line warped back into its
  place; `DeviceCollator.quad_windows` and `DeviceExporter.scene_quads` are the same on the GPU (csrc/quads.hip), byte for byte.
* `poly_check` / `poly_matrices` / `poly_paste_host` / `poly_compose_host` / `super_resolve_polys_host` (tatt_amd/polys.py, re-exported
  here) take POLYGONS of 2 N points, a detector's curved text: straightened strip by strip, the finished line pasted back with exact
  seams; `DeviceCollator.poly_windows` and `DeviceExporter.scene_polys` are the same on the GPU (csrc/polys.hip), byte for byte.
* `LmdbRecords` reads the reference's lmdb record layout (`lmdbDataset_real`, dataset/dataset.py:565-686): keys `num-samples`,
  `label-%09d`, `image_hr-%09d`, `image_lr-%09d` (1-based), image bytes decoded by PIL to RGB, the label filtered by `str_filt`.
  It takes any object with the lmdb transaction's `get(key)`; `open_lmdb` wraps a real environment when the `lmdb` package is there
  (it is not in this image: the record logic is tested against an in-memory mapping).
Host-side data plumbing (PIL / numpy), not part of the GPU path: torch.save / torch.load / PIL are file-format code; all arithmetic of
the training step stays in the HIP kernels.
"""
from __future__ import annotations

import os
import string
from typing import Iterable, Optional, Sequence

import torch

ALPHABET = "0123456789abcdefghijklmnopqrstuvwxyz"          # class 0 is the CTC blank "-" (reference utils/metrics.py:71)


def _unwrap(m):
    return m.module if hasattr(m, "module") and isinstance(getattr(m, "module"), torch.nn.Module) else m


def save_checkpoint(netG_list: Sequence[torch.nn.Module], epoch: int, iters: int, best_acc_dict, best_model_info, is_best: bool,
                    converge_list, ckpt_path: str, *, arch: str = "tatt", batch_size: int = 48, voc_type: str = "all",
                    scale_factor: int = 2, recognizer=None, prefix: str = "acc"):
    """reference TextBase.save_checkpoint (interfaces/base.py:621-672); returns the list of files written."""
    os.makedirs(ckpt_path, exist_ok=True)
    written = []
    for i, net in enumerate(netG_list):
        netG = _unwrap(net)
        save_dict = {
            "state_dict_G": {k: v.detach().cpu() for k, v in netG.state_dict().items()},
            "info": {"arch": arch, "iters": iters, "epochs": epoch, "batch_size": batch_size, "voc_type": voc_type,
                     "up_scale_factor": scale_factor},
            "best_history_res": best_acc_dict,
            "best_model_info": best_model_info,
            "param_num": sum(p.nelement() for p in netG.parameters()),
            "converge": converge_list,
        }
        name = ("model_best_%s_%d.pth" % (prefix, i)) if is_best else "checkpoint.pth"
        torch.save(save_dict, os.path.join(ckpt_path, name))
        written.append(os.path.join(ckpt_path, name))
    if recognizer is not None:
        recs = recognizer if isinstance(recognizer, (list, tuple)) else [recognizer]
        for i, r in enumerate(recs):
            if isinstance(recognizer, (list, tuple)):
                name = ("recognizer_best_%s_%d.pth" % (prefix, i)) if is_best else "recognizer_%d.pth" % i
            else:
                name = "recognizer_best.pth" if is_best else "recognizer.pth"
            torch.save({k: v.detach().cpu() for k, v in _unwrap(r).state_dict().items()}, os.path.join(ckpt_path, name))
            written.append(os.path.join(ckpt_path, name))
    return written


def _strip_module(sd):
    return {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}


def load_generator(model: torch.nn.Module, resume: str, iter_: int = 0, strict: Optional[bool] = None):
    """reference TextBase.generator_init resume branch (interfaces/base.py:398-443).  `resume` is a checkpoint file or a directory
    holding model_best_acc_<iter_>.pth; directories load with strict=False like the reference, files strictly.  Returns the
    checkpoint's 'info' dict (or None for a bare state_dict)."""
    is_dir = os.path.isdir(resume)
    path = os.path.join(resume, "model_best_acc_%d.pth" % iter_) if is_dir else resume
    blob = torch.load(path, map_location="cpu")
    sd = blob["state_dict_G"] if isinstance(blob, dict) and "state_dict_G" in blob else blob
    target = _unwrap(model)
    target.load_state_dict(_strip_module(sd), strict=(not is_dir) if strict is None else strict)
    return blob.get("info") if isinstance(blob, dict) and "state_dict_G" in blob else None


def stretch_label(word: str, max_len: int = 26) -> str:
    """The reference's label layout (dataset/dataset.py:2015-2034): lower-cased; words of 2..25 characters are spread over the
    26 prior steps by inserting int((26 - len) / (len - 1)) blanks between neighbouring characters; longer words are cut."""
    word = word.lower()
    if len(word) <= 1:
        return word
    if len(word) < max_len:
        pad = int((max_len - len(word)) / (len(word) - 1))
        return word[0] + "".join("-" * pad + ch for ch in word[1:])
    return word[:max_len]


def collate_labels(label_strs: Sequence[str], alphabet: str = ALPHABET, max_len: int = 26):
    """-> (label_vecs (B, len(alphabet)+1, 1, max_len) one-hot float, weighted_mask (sum of label lengths,) long, weighted_tics (B,) long)
    exactly as alignCollate_realWTLAMask builds them (dataset/dataset.py:2009-2063): characters outside the alphabet are dropped, a
    word with no valid character becomes a single blank (class 0) with tic 0."""
    d2a = "-" + alphabet
    a2d = {ch: i for i, ch in enumerate(d2a)}
    alsize = len(d2a)
    out = torch.zeros(len(label_strs), max_len, alsize)
    masks, tics = [], []
    for b, word in enumerate(label_strs):
        ids = [a2d[ch] for ch in stretch_label(word, max_len) if ch in a2d]
        if ids:
            masks.extend(ids)
            out[b, torch.arange(len(ids)), torch.tensor(ids)] = 1.0
            tics.append(1)
        else:
            masks.append(0)
            out[b, 0, 0] = 1.0
            tics.append(0)
    return out.unsqueeze(1).permute(0, 3, 1, 2).contiguous(), torch.tensor(masks).long(), torch.tensor(tics)


def collate_batch(samples, device=None, alphabet: str = ALPHABET):
    """samples: iterable of (img_HR, img_lr, img_HRy, img_lry, label_str) with the images already tensors of their final size
    ((4 or 3, H, W) float in [0, 1]) -> the tuple of the reference's collate function (dataset/dataset.py:2077):
    (images_HR, images_pseudoLR = None, images_lr, images_HRy, images_lry, label_strs, label_vecs, weighted_mask, weighted_tics),
    image stacks and label_vecs on `device` (the loop's `.to(self.device)`, interfaces/super_resolution.py:700-707)."""
    hr, lr, hry, lry, labels = zip(*samples)
    st = lambda ts: torch.stack([torch.as_tensor(t) for t in ts], 0).to(device) if device is not None else torch.stack(
        [torch.as_tensor(t) for t in ts], 0)
    vecs, masks, tics = collate_labels(labels, alphabet)
    return st(hr), None, st(lr), st(hry), st(lry), tuple(labels), (vecs.to(device) if device is not None else vecs), masks, tics


def _to_tensor(img):
    """torchvision.transforms.ToTensor for a uint8 PIL image: (H, W[, C]) uint8 -> (C, H, W) float32 in [0, 1]"""
    import numpy as np
    a = np.asarray(img)
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(np.array(a.transpose(2, 0, 1))).float().div(255)                  # (np.array: a writable, contiguous copy)


def resize_normalize(img, size, mask: bool = False):
    """reference `resizeNormalize(size, mask)(img)` (dataset/dataset.py:1266-1319, the ratio_keep / aug branches unused by the TATT
    loaders): img: PIL image; size = (width, height).  Bicubic resize, ToTensor, and with `mask` a fourth plane that is 1 where the
    gray value does not exceed the image's mean gray value (`mask.point(lambda x: 0 if x > thres else 255)`) -- dark text on a
    bright background comes out as 1."""
    import numpy as np
    from PIL import Image
    img = img.resize(tuple(size), Image.BICUBIC)
    t = _to_tensor(img)
    if mask:
        m = img.convert("L")
        thres = np.array(m).mean()
        m = m.point(lambda v: 0 if v > thres else 255)
        t = torch.cat((t, _to_tensor(m)), 0)
    return t


def collate_pil_batch(samples, imgH: int = 32, imgW: int = 128, down_sample_scale: int = 2, mask: bool = True, device=None,
                      alphabet: str = ALPHABET):
    """samples: iterable of (img_HR, img_lr, img_HRy, img_lry, label_str) with PIL images, as `lmdbDataset_real.__getitem__` yields
    them -> the reference's batch tuple (alignCollate_realWTLAMask.__call__, dataset/dataset.py:1980-2077): HR images resized to
    (imgW, imgH), LR images to (imgW, imgH) / down_sample_scale, each with its mask plane."""
    hr_size, lr_size = (imgW, imgH), (imgW // down_sample_scale, imgH // down_sample_scale)
    rows = [(resize_normalize(hr, hr_size, mask), resize_normalize(lr, lr_size, mask), resize_normalize(hry, hr_size, mask),
             resize_normalize(lry, lr_size, mask), lab) for hr, lr, hry, lry, lab in samples]
    return collate_batch(rows, device=device, alphabet=alphabet)


def rgb_to_yuv_u8(rgb):
    """cv2.cvtColor(img, cv2.COLOR_RGB2YUV) for uint8 (dataset/dataset.py:668-674: the `images_lry` / `images_HRy` members of a sample,
    read by the loop only with --y_domain, which the TATT recipes do not set): Y = 0.299 R + 0.587 G + 0.114 B, U = 0.492 (B - Y) + 128,
    V = 0.877 (R - Y) + 128, rounded and saturated.  (cv2 evaluates this in 14-bit fixed point; results may differ from it by one
    count -- cv2 is not in this image, so this member is NOT pinned against the reference.)"""
    import numpy as np
    a = np.asarray(rgb).astype(np.float64)
    y = 0.299 * a[..., 0] + 0.587 * a[..., 1] + 0.114 * a[..., 2]
    u = 0.492 * (a[..., 2] - y) + 128.0
    v = 0.877 * (a[..., 0] - y) + 128.0
    return np.clip(np.rint(np.stack([y, u, v], -1)), 0, 255).astype(np.uint8)


class LmdbRecords:
    """The reference's lmdb record layout read through a transaction-like object (`get(bytes) -> bytes or None`), reference
    `lmdbDataset_real` (dataset/dataset.py:565-686): `num-samples` holds the count, sample i (1-based) is `image_hr-%09d`,
    `image_lr-%09d` (encoded image files) and `label-%09d` (utf-8).  __getitem__(index) -> (img_HR, img_lr, img_HRy, img_lry,
    label_str) with PIL images, the label passed through `str_filt(word, voc_type)`.
    Bad records, exactly as the reference behaves (dataset/dataset.py:640-686): its `except IOError or len(word) > self.max_len` catches
    IOError ONLY (the `or` picks the class), so an over-long label is RETURNED, not skipped (`max_len` is kept as an attribute, unused as
    upstream); on an unreadable image it returns `self[index + 1]` AFTER `index += 1`, i.e. 0-based item i falls through to item i + 2 --
    one record further than it looks.  Running past the last record raises IndexError (upstream: an assertion / a missing key).
    NOT exercised against a real lmdb environment: the `lmdb` package is absent from this image (tests use an in-memory mapping)."""

    def __init__(self, txn, voc_type: str = "upper", max_len: int = 100):
        self.txn, self.voc_type, self.max_len = txn, voc_type, max_len
        n = txn.get(b"num-samples")
        if n is None:
            raise KeyError("lmdb environment without a num-samples record")
        self.n = int(n)

    def __len__(self):
        return self.n

    def _image(self, key):
        import io as _io
        from PIL import Image
        buf = self.txn.get(key)
        if buf is None:
            raise IOError("missing record %r" % key)
        return Image.open(_io.BytesIO(buf)).convert("RGB")

    def __getitem__(self, index):
        from PIL import Image
        if not 0 <= index < self.n:
            raise IndexError(index)
        while index < self.n:
            i = index + 1                                            # 1-based record
            try:
                hr, lr = self._image(b"image_hr-%09d" % i), self._image(b"image_lr-%09d" % i)
            except (IOError, OSError):
                index += 2                                           # the reference's `return self[index + 1]` after `index += 1`
                continue
            word = self.txn.get(b"label-%09d" % i)
            word = " " if word is None else word.decode()
            hry, lry = Image.fromarray(rgb_to_yuv_u8(hr)), Image.fromarray(rgb_to_yuv_u8(lr))
            return hr, lr, hry, lry, str_filt(word, self.voc_type)
        raise IndexError("no readable record at or after the requested index")


def open_lmdb(root: str, **kw) -> LmdbRecords:
    """`lmdbDataset_real(root)`: opens the environment read-only like the reference (dataset/dataset.py:576-583).  Needs the `lmdb`
    package (absent from this image: ImportError says so)."""
    import lmdb                                                  # noqa: F401 -- optional dependency of the data pipeline only
    env = lmdb.open(root, max_readers=1, readonly=True, lock=False, readahead=False, meminit=False)
    return LmdbRecords(env.begin(write=False), **kw)


def ctc_greedy_decode(logits: torch.Tensor, alphabet: str = ALPHABET) -> list:
    """(T, B, C) recogniser outputs -> B strings: arg-max per step, repeats merged, blanks dropped (reference get_string_crnn,
    utils/metrics.py:71-92).  The arg-max is an index operation on a (T, B) grid; the strings are built on the host."""
    d2a = "-" + alphabet
    idx = logits.detach().permute(1, 0, 2).argmax(2).cpu().tolist()
    out = []
    for row in idx:
        s, last = "", ""
        for i in row:
            if d2a[i] != last:
                if i != 0:
                    s += d2a[i]
                    last = d2a[i]
                else:
                    last = ""
        out.append(s)
    return out


def str_filt(s: str, voc_type: str = "lower") -> str:
    """reference utils/util.py:12-32 for the Latin vocabularies ('digit', 'lower', 'upper', 'all')."""
    alpha = {"digit": string.digits, "lower": string.digits + string.ascii_lowercase, "upper": string.digits + string.ascii_letters,
             "all": string.digits + string.ascii_letters + string.punctuation}[voc_type]
    if voc_type == "lower":
        s = s.lower()
    return "".join(ch for ch in s if ch in alpha)


def edit_distance(a: str, b: str) -> int:
    """Levenshtein distance with unit costs between two strings: what the reference's `editdistance.eval` returns
    (interfaces/super_resolution.py:1531-1556).  Pure Python, the textbook row-by-row DP; it is the specification of
    tatt_ctc_greedy_score's distance."""
    if len(a) < len(b):
        a, b = b, a
    row = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        prev, row[0] = row[0], i
        for j, cb in enumerate(b, 1):
            prev, row[j] = row[j], min(row[j] + 1, row[j - 1] + 1, prev + (ca != cb))
    return row[len(b)]


LABEL_CAP = 64            # most characters of a filtered label the edit-distance metrics score (the score kernel's label width)


@torch.no_grad()
def evaluate(model: torch.nn.Module, batches: Iterable, prior_fn=None, recognizer=None, voc_type: str = "lower",
             full_metrics: bool = False):
    """Metric part of the reference's eval loop: for every (images_lr, images_hr[, text_prior[, label_strs]]) batch run the
    generator in eval mode and accumulate calculate_psnr / SSIM of SR vs HR on the first three channels
    (interfaces/super_resolution.py:1454-1455).  With a `recognizer` (tatt_amd.CRNN, the reference's --test_model CRNN) and label
    strings in the batch, also the recognition accuracies of the SR, LR and HR images (:1374-1396,1527-1558,1662-1664).
    Returns {'psnr', 'ssim', 'n_batches'[, 'accuracy', 'accuracy_lr', 'accuracy_hr', 'n_images']} (python floats).
    full_metrics=True adds the rest of the reference's report: 'psnr_lr' / 'ssim_lr', the bicubic baseline
    F.interpolate(images_lr, hr_size, mode="bicubic") against HR (:1417-1418,1452), and with a recogniser 'ned' / 'ned_lr' / 'ned_hr',
    the mean of edit_distance(pred, label) / (max(len(pred), len(label)) + 1e-10) over the images (:1531-1556,1633-1635; both
    strings through str_filt), and 'ned_skipped': the images whose filtered label has more than LABEL_CAP characters, which the
    means leave out (the same rule as the device path, `infer.evaluate_session`).
    A `tatt_amd.ASTER` recogniser (--test_model ASTER) is read through parse_aster_data, beam search and get_string_aster instead and
    returns the same keys (`_evaluate_aster`: the ids stay on the device, one copy at the end).  A `tatt_amd.MORAN` recogniser
    (--test_model MORAN) is read through parse_moran_data, 20 greedy steps of the L2R decoder and get_string_moran, in the same way."""
    from .losses import SSIM, calculate_psnr
    from .crnn import bicubic_resize, parse_crnn_data
    from .aster import ASTER
    from .moran import MORAN
    if isinstance(recognizer, ASTER):
        return _evaluate_aster(model, batches, prior_fn, recognizer, voc_type, full_metrics)
    if isinstance(recognizer, MORAN):
        return _evaluate_moran(model, batches, prior_fn, recognizer, voc_type, full_metrics)
    was_training = model.training
    model.eval()
    ssim = SSIM()
    psnr_sum = torch.zeros((), device=next(model.parameters()).device)
    ssim_sum = torch.zeros_like(psnr_sum)
    psnr_lr_sum, ssim_lr_sum = torch.zeros_like(psnr_sum), torch.zeros_like(psnr_sum)
    n = 0
    correct = {"sr": 0, "lr": 0, "hr": 0}
    ned = {"sr": 0.0, "lr": 0.0, "hr": 0.0}
    n_img = n_scored = n_skipped = 0
    rec_was_training = recognizer.training if recognizer is not None else False
    if recognizer is not None:
        recognizer.eval()
    for batch in batches:
        lr, hr = batch[0], batch[1]
        tp = batch[2] if len(batch) > 2 and batch[2] is not None else (prior_fn(lr) if prior_fn is not None else None)
        labels = batch[3] if len(batch) > 3 else None
        out = model(lr, tp) if tp is not None else model(lr)
        sr = out[0] if isinstance(out, tuple) else out
        psnr_sum += calculate_psnr(sr[:, :3], hr[:, :3])
        ssim_sum += ssim(sr[:, :3], hr[:, :3])
        if full_metrics:
            up = bicubic_resize(lr[:, :3], hr.shape[-2:])
            psnr_lr_sum += calculate_psnr(up, hr[:, :3])
            ssim_lr_sum += ssim(up, hr[:, :3])
        n += 1
        if recognizer is not None and labels is not None:
            want = [str_filt(t, voc_type) for t in labels]
            scored = [len(t) <= LABEL_CAP for t in want]
            for name, img in (("sr", sr), ("lr", lr), ("hr", hr)):
                pred = ctc_greedy_decode(recognizer(parse_crnn_data(img[:, :3].contiguous())))
                pred = [str_filt(p, voc_type) for p in pred]
                correct[name] += sum(p == t for p, t in zip(pred, want))
                if full_metrics:
                    ned[name] += sum(edit_distance(p, t) / (max(len(p), len(t)) + 1e-10) for p, t, ok in zip(pred, want, scored) if ok)
            n_img += len(labels)
            n_scored += sum(scored)
            n_skipped += len(scored) - sum(scored)
    model.train(was_training)
    if recognizer is not None:
        recognizer.train(rec_was_training)               # e.g. TextPriorSR.tpg under training: BatchNorm must not stay in eval mode
    res = {"psnr": float(psnr_sum) / max(n, 1), "ssim": float(ssim_sum) / max(n, 1), "n_batches": n}
    if full_metrics:
        res.update(psnr_lr=float(psnr_lr_sum) / max(n, 1), ssim_lr=float(ssim_lr_sum) / max(n, 1))
    if n_img:
        res.update(accuracy=round(correct["sr"] / n_img, 4), accuracy_lr=round(correct["lr"] / n_img, 4),
                   accuracy_hr=round(correct["hr"] / n_img, 4), n_images=n_img)
        if full_metrics:
            res.update(ned=ned["sr"] / (n_scored + 1e-10), ned_lr=ned["lr"] / (n_scored + 1e-10), ned_hr=ned["hr"] / (n_scored + 1e-10),
                       ned_skipped=n_skipped)
    return res


@torch.no_grad()
def _evaluate_aster(model, batches, prior_fn, recognizer, voc_type, full_metrics):
    """`evaluate` with an ASTER recogniser (the reference's --test_model ASTER: parse_aster_data -> beam search -> get_string_aster, both
    strings through str_filt; interfaces/super_resolution.py:1374-1396).  The ids of every batch stay on the device; ONE copy at the end
    brings them and the image metrics back, and the strings are decoded on the host from it."""
    from .aster import AsterInfo, get_string_aster, parse_aster_data
    info = getattr(recognizer, "info", None)
    if info is None:
        voc = {13: "digit", 39: "lower", 65: "upper", 97: "all"}.get(recognizer.rec_num_classes)
        if voc is None:
            raise ValueError("io.evaluate: no vocabulary has %d classes (digit 13, lower 39, upper 65, all 97); set recognizer.info to "
                             "the AsterInfo it was trained with" % recognizer.rec_num_classes)
        info = AsterInfo(voc)
    elif info.rec_num_classes != recognizer.rec_num_classes:
        raise ValueError("io.evaluate: recognizer.info has %d classes, the recogniser %d" % (info.rec_num_classes, recognizer.rec_num_classes))
    return _evaluate_ids(model, batches, prior_fn, recognizer, voc_type, full_metrics,
                         lambda img: recognizer.read(parse_aster_data(img[:, :3]), "beam")[0], recognizer.max_len_labels,
                         lambda rows: get_string_aster(rows, info))


@torch.no_grad()
def _evaluate_moran(model, batches, prior_fn, recognizer, voc_type, full_metrics):
    """`evaluate` with a MORAN recogniser (the reference's --test_model MORAN: parse_moran_data -> the model in test mode -> the arg-max
    of the L2R rows -> the alphabet's characters cut at the first '$', both strings through str_filt;
    interfaces/super_resolution.py:1401-1405).  `MORAN.read` runs the L2R decoder only (the reference computes the R2L rows and throws
    them away).  One host copy, as in `_evaluate_aster`."""
    from .moran import ALPHABET, MAX_ITER, get_string_moran, parse_moran_data
    if recognizer.nclass != len(ALPHABET) or recognizer.nc != 1:
        raise ValueError("io.evaluate: the MORAN recogniser must read one channel and have %d classes (0-9a-z$), got nc=%d, nclass=%d"
                         % (len(ALPHABET), recognizer.nc, recognizer.nclass))
    return _evaluate_ids(model, batches, prior_fn, recognizer, voc_type, full_metrics,
                         lambda img: recognizer.read(parse_moran_data(img[:, :3], recognizer.targetW)[0], MAX_ITER)[0], MAX_ITER,
                         get_string_moran)


def _evaluate_ids(model, batches, prior_fn, recognizer, voc_type, full_metrics, read, L, strings):
    """the loop `_evaluate_aster` and `_evaluate_moran` share: read(img) -> (B, L) int32 ids on the device, strings(rows) -> B strings"""
    from .losses import SSIM, calculate_psnr
    from .crnn import bicubic_resize
    was_training, rec_was_training = model.training, recognizer.training
    model.eval()
    recognizer.eval()
    ssim = SSIM()
    dev = next(model.parameters()).device
    sums = torch.zeros(4, device=dev)                  # psnr, ssim, psnr_lr, ssim_lr
    n = 0
    ids, all_labels = {"sr": [], "lr": [], "hr": []}, []
    for batch in batches:
        lr, hr = batch[0], batch[1]
        tp = batch[2] if len(batch) > 2 and batch[2] is not None else (prior_fn(lr) if prior_fn is not None else None)
        labels = batch[3] if len(batch) > 3 else None
        out = model(lr, tp) if tp is not None else model(lr)
        sr = out[0] if isinstance(out, tuple) else out
        sums[0] += calculate_psnr(sr[:, :3], hr[:, :3])
        sums[1] += ssim(sr[:, :3], hr[:, :3])
        if full_metrics:
            up = bicubic_resize(lr[:, :3], hr.shape[-2:])
            sums[2] += calculate_psnr(up, hr[:, :3])
            sums[3] += ssim(up, hr[:, :3])
        n += 1
        if labels is not None:
            for name, img in (("sr", sr), ("lr", lr), ("hr", hr)):
                ids[name].append(read(img))
            all_labels += list(labels)
    model.train(was_training)
    recognizer.train(rec_was_training)
    flat = [t.reshape(-1) for k in ("sr", "lr", "hr") for t in ids[k]]
    host = torch.cat(flat + [sums.view(torch.int32)]).cpu()                    # the evaluation's one host synchronisation
    s4 = host[-4:].view(torch.float32).tolist()
    res = {"psnr": s4[0] / max(n, 1), "ssim": s4[1] / max(n, 1), "n_batches": n}
    if full_metrics:
        res.update(psnr_lr=s4[2] / max(n, 1), ssim_lr=s4[3] / max(n, 1))
    n_img = len(all_labels)
    if n_img:
        want = [str_filt(t, voc_type) for t in all_labels]
        scored = [len(t) <= LABEL_CAP for t in want]
        acc, ned = {}, {}
        off = 0
        for name in ("sr", "lr", "hr"):
            rows = host[off:off + n_img * L].view(n_img, L)
            off += n_img * L
            pred = [str_filt(p, voc_type) for p in strings(rows)]
            acc[name] = sum(p == t for p, t in zip(pred, want))
            ned[name] = sum(edit_distance(p, t) / (max(len(p), len(t)) + 1e-10) for p, t, ok in zip(pred, want, scored) if ok)
        res.update(accuracy=round(acc["sr"] / n_img, 4), accuracy_lr=round(acc["lr"] / n_img, 4), accuracy_hr=round(acc["hr"] / n_img, 4),
                   n_images=n_img)
        if full_metrics:
            n_scored = sum(scored)
            res.update(ned=ned["sr"] / (n_scored + 1e-10), ned_lr=ned["lr"] / (n_scored + 1e-10), ned_hr=ned["hr"] / (n_scored + 1e-10),
                       ned_skipped=len(scored) - n_scored)
    return res


# ---- batch collation on the device (csrc/collate.hip) -----------------------------------------------------------------------------
COLLATE_DESC = 8          # ints per descriptor row of tatt_collate_images (include/tatt_hip.h)
_COLLATE_ALIGN = 16


def collate_limits():
    """tatt_collate_limits: {'rows', 'cols', 'inter_bytes', 'oh', 'ow'} -- the sources the device resampler takes (larger ones are resized
    by PIL on the host and only converted on the device) and the largest target size.  A host-only entry: needs no GPU."""
    import ctypes
    from ._lib import LIB
    out = (ctypes.c_int * 5)()
    if LIB.tatt_collate_limits(out) != 0:
        raise RuntimeError("tatt_collate_limits failed")
    return dict(zip(("rows", "cols", "inter_bytes", "oh", "ow"), (int(v) for v in out)))


def collate_plan(images, sizes, mask: bool = True, limits=None):
    """Host half of `DeviceCollator`, without a device: images: RGB PIL images, sizes: their (width, height) targets.
    -> (arrays, desc, nbytes, out_floats): arrays[i] the (H, W, 3) uint8 pixels of item i (`np.asarray(img)`; an image beyond `limits` is
    replaced by its PIL-resized version, which the device then only converts: exact by construction), desc (n, COLLATE_DESC) int32 rows
    [source byte offset (16-byte aligned, counted from the end of the descriptor table's block), H_src, W_src, OH, OW, mask, float offset
    of the item's planes, 0] with the planes of the items one after the other, nbytes the packed size of the sources, out_floats the size
    of the output."""
    import numpy as np
    from PIL import Image
    lim = limits if limits is not None else collate_limits()
    n = len(images)
    desc = np.zeros((n, COLLATE_DESC), np.int32)
    arrays, off, out_off, planes = [], 0, 0, 3 + int(bool(mask))
    for i, (img, (ow, oh)) in enumerate(zip(images, sizes)):
        if getattr(img, "mode", None) != "RGB":
            raise ValueError("DeviceCollator takes RGB PIL images (Image.open(..).convert('RGB')); item %d is %r" % (
                i, getattr(img, "mode", type(img).__name__)))
        if not (1 <= oh <= lim["oh"] and 1 <= ow <= lim["ow"]):
            raise ValueError("tatt_collate_images takes targets up to %d x %d (got %d x %d)" % (lim["oh"], lim["ow"], oh, ow))
        ws, hs = img.size
        if hs > lim["rows"] or ws > lim["cols"] or (ws != ow and hs * ow * 3 > lim["inter_bytes"]):
            img = img.resize((ow, oh), Image.BICUBIC)
            ws, hs = ow, oh
        a = np.asarray(img)
        arrays.append(a)
        desc[i] = (off, hs, ws, oh, ow, int(bool(mask)), out_off, 0)
        off += -(-a.size // _COLLATE_ALIGN) * _COLLATE_ALIGN
        out_off += planes * oh * ow
        if off >= 2 ** 31 or out_off >= 2 ** 31:
            raise ValueError("DeviceCollator: the batch does not fit 32-bit offsets")
    return arrays, desc, off, out_off


def collate_fill(flat, arrays, desc, vecs):
    """Write one staging slot: flat: a writable 1-D uint8 array (the pinned slot, or any buffer) -> (head, pix, used).  Layout, each
    block 16-byte aligned: descriptor table (desc rows as int32) at 0 | label_vecs as float32 at `head` | the pixels of item i at
    `pix + desc[i, 0]`; `used` bytes in all (`collate_fill(None, ...)` only computes the three offsets)."""
    import numpy as np
    nvec = int(np.prod(vecs.shape))
    head = -(-desc.nbytes // _COLLATE_ALIGN) * _COLLATE_ALIGN
    pix = head + -(-nvec * 4 // _COLLATE_ALIGN) * _COLLATE_ALIGN
    used = pix + (int(desc[-1, 0]) + -(-arrays[-1].size // _COLLATE_ALIGN) * _COLLATE_ALIGN if len(arrays) else 0)
    if flat is not None:
        flat[:desc.nbytes].view(np.int32)[:] = desc.reshape(-1)
        flat[head:head + nvec * 4].view(np.float32)[:] = np.asarray(vecs, dtype=np.float32).reshape(-1)
        for a, row in zip(arrays, desc):
            o = pix + int(row[0])
            flat[o:o + a.size] = a.reshape(-1)
    return head, pix, used


class _Limits:
    """the limit tables of the C layer, each read once per instance: `self._limits` (declared by the class that uses this) maps a
    `*_limits` function (`collate_limits`, `line_limits`, ...) to what it returned"""

    def _lim(self, limits):
        if limits not in self._limits:
            self._limits[limits] = limits()
        return self._limits[limits]


def _ptrs(base, hbase, off):
    """a table `off` bytes into the device buffer and into its pinned slot: the (device, host) pointer pair the launches take"""
    import ctypes
    return ctypes.c_void_p(base + off), ctypes.c_void_p(hbase + off)


class DeviceCollator(_Limits):
    """`collate_pil_batch` with the image stacks built on the GPU: collate(samples) takes what `collate_pil_batch` takes ((img_HR, img_lr,
    img_HRy, img_lry, label_str) with RGB PIL images) and returns the same 9-tuple with `images_HR` / `images_lr` BIT FOR BIT equal to the
    host path's, on `device`.  `want_yuv=False` (the TATT recipes never read those members): `images_HRy` / `images_lry` are None; True:
    they go through the same launch as two more items per sample.  Labels go through `collate_labels`.
    The host does one packing pass over raw bytes (`collate_plan`) into a slot of a ring of pinned staging buffers -- descriptor table and
    pixels together -- and enqueues ONE non-blocking copy to a persistent device buffer and ONE launch (tatt_collate_images: resize +
    ToTensor + mask for every image) on the current stream; it never waits for the device.  A slot is rewritten only after the event
    recorded behind its previous copy (the discipline of `TextPriorSR.set_labels`); a batch that outgrows the slots re-allocates them after
    waiting for those events.  The image stacks are views of one freshly allocated tensor per call.  Decoding stays with the caller.
    Every entry point goes through `_stage`, the one place that holds this discipline."""

    def __init__(self, imgH: int = 32, imgW: int = 128, down_sample_scale: int = 2, mask: bool = True, device="cuda",
                 want_yuv: bool = False, ring: int = 3, alphabet: str = ALPHABET):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tatt_amd kernels need tensors on an AMD GPU (HIP device); got %s. "
                               "There is no CPU fallback in the product path (collate_pil_batch is the host path)." % self.device)
        if ring < 1:
            raise ValueError("DeviceCollator: ring must be at least 1")
        self.hr_size, self.lr_size = (imgW, imgH), (imgW // down_sample_scale, imgH // down_sample_scale)
        self.mask, self.want_yuv, self.ring, self.alphabet = bool(mask), bool(want_yuv), int(ring), alphabet
        self._limits = {}
        self._host, self._events, self._dev_buf, self._i, self._last = [], [], None, 0, None

    def plan(self, samples):
        """-> (collate_plan(...) of the batch's items, label strings, members): items ordered HR x B, lr x B[, HRy x B, lry x B]"""
        hr, lr, hry, lry, labels = zip(*samples)
        members = [(hr, self.hr_size), (lr, self.lr_size)] + ([(hry, self.hr_size), (lry, self.lr_size)] if self.want_yuv else [])
        images = [im for ims, _ in members for im in ims]
        sizes = [size for ims, size in members for _ in ims]
        return collate_plan(images, sizes, self.mask, self._lim(collate_limits)), labels, members

    def _slot(self, need):
        """the next staging slot (a pinned uint8 tensor of at least `need` bytes), free to be written"""
        if not self._host or self._host[0].numel() < need:
            for ev in self._events + ([self._last[1]] if self._last is not None else []):
                if ev is not None:
                    ev.synchronize()
            cap = -(-need * 3 // 2 // 4096) * 4096
            self._host = [torch.empty(cap, dtype=torch.uint8, pin_memory=True) for _ in range(self.ring)]
            self._events = [None] * self.ring
            self._dev_buf = torch.empty(cap, dtype=torch.uint8, device=self.device)
        k = self._i % self.ring
        self._i += 1
        if self._events[k] is not None:
            self._events[k].synchronize()
        return k, self._host[k]

    def _stage(self, need, used, fill, launch):
        """One call's staging step, on the current stream: take a slot and a device buffer of at least `need` bytes, fill(flat) the slot
        (flat: its writable uint8 array), copy its first `used` bytes to the device (ONE non-blocking copy), record the slot's event, run
        launch(base, hbase) -- the device buffer's and the slot's address; it enqueues the call's launches and allocates their output --
        and record the event the next call on ANOTHER stream waits for.  -> what `launch` returns.  Never waits for the device (but for a
        slot's own event, and to re-allocate outgrown slots: `_slot`)."""
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream()
            moved = self._last is not None and self._last[0] != stream
            if moved:
                stream.wait_event(self._last[1])             # the one device buffer: the previous call's launch still reads it
            k, host = self._slot(need)
            if moved:
                self._dev_buf.record_stream(stream)
            fill(host.numpy())
            self._dev_buf[:used].copy_(host[:used], non_blocking=True)
            ev = self._events[k] = self._events[k] if self._events[k] is not None else torch.cuda.Event()
            ev.record(stream)
            out = launch(self._dev_buf.data_ptr(), host.data_ptr())
            done = self._last[1] if self._last is not None else torch.cuda.Event()
            done.record(stream)
            self._last = (stream, done)
        return out

    def __call__(self, samples):
        from . import ops
        samples = list(samples)
        (arrays, desc, nbytes, out_floats), labels, members = self.plan(samples)
        B, n = len(samples), len(arrays)
        vecs, masks, tics = collate_labels(labels, self.alphabet)
        vecs_np = vecs.numpy()
        head, pix, used = collate_fill(None, arrays, desc, vecs_np)

        def launch(base, hbase):
            out = torch.empty(out_floats + vecs.numel(), dtype=torch.float32, device=self.device)
            ops.call("tatt_collate_images", _ptrs(base, hbase, pix)[0], nbytes, *_ptrs(base, hbase, 0), n, ops.P(out), out_floats,
                     ops.stream())
            vecs_dev = out[out_floats:].view(vecs.shape)     # (device-to-device, behind the one host-to-device copy)
            vecs_dev.copy_(self._dev_buf[head:head + vecs.numel() * 4].view(torch.float32).view(vecs.shape), non_blocking=True)
            return out, vecs_dev
        out, vecs_dev = self._stage(used, used, lambda flat: collate_fill(flat, arrays, desc, vecs_np), launch)
        C, stacks, o = 3 + int(self.mask), [], 0
        for _, (w, h) in members:
            stacks.append(out[o:o + B * C * h * w].view(B, C, h, w))
            o += B * C * h * w
        return (stacks[0], None, stacks[1], stacks[2] if self.want_yuv else None, stacks[3] if self.want_yuv else None, tuple(labels),
                vecs_dev, masks, tics)

    def _windows(self, kernel, pix, nbytes, n, out_floats):
        """-> the launch of `_stage` for ONE window kernel (tatt_collate_images, tatt_line_windows and tatt_scene_windows share an
        argument list): the sources `pix` bytes into the buffer, the descriptor table of n rows at its start"""
        from . import ops

        def launch(base, hbase):
            out = torch.empty(out_floats, dtype=torch.float32, device=self.device)
            ops.call(kernel, _ptrs(base, hbase, pix)[0], nbytes, *_ptrs(base, hbase, 0), n, ops.P(out), out_floats, ops.stream())
            return out
        return launch

    def stack(self, images, size):
        """RGB PIL images, size = (width, height) -> ONE (n, 3 + mask, height, width) stack on the device, bit for bit
        `torch.stack([resize_normalize(im, size, mask) for im in images])`: the plan / fill / launch of `__call__` without the sample
        tuples and the labels (what `tatt_amd.infer.SuperResolver` feeds its sessions with).  Never waits for the device."""
        import numpy as np
        images = list(images)
        arrays, desc, nbytes, out_floats = collate_plan(images, [tuple(size)] * len(images), self.mask, self._lim(collate_limits))
        none = np.zeros(0, np.float32)
        _, pix, used = collate_fill(None, arrays, desc, none)
        out = self._stage(used, used, lambda flat: collate_fill(flat, arrays, desc, none),
                          self._windows("tatt_collate_images", pix, nbytes, len(arrays), out_floats))
        return out.view(len(images), 3 + int(self.mask), size[1], size[0])

    def windows(self, images, stride: int = 32):
        """RGB PIL images (text lines of any width) -> (stack, lines): ONE (n_windows, 3 + mask, h, w) stack on the device holding the
        windows of every line at the collator's LR size, lines in input order and windows left to right, bit for bit
        `torch.cat([line_windows_host(im, (h, w), stride, mask) for im in images])`; lines[i] = Line(wl, starts, first window index), what
        `DeviceExporter.lines` needs.  One upload per line (not per window), one copy, one launch (tatt_line_windows) through the ring of
        `stack`.  Never waits for the device."""
        w, h = self.lr_size
        arrays, desc, lines, nbytes, out_floats = lines_plan(list(images), (h, w), stride, self.mask, self._lim(line_limits))
        if not lines:
            raise ValueError("DeviceCollator.windows: no images")
        pix, used = lines_fill(None, arrays, desc)
        out = self._stage(used, used, lambda flat: lines_fill(flat, arrays, desc),
                          self._windows("tatt_line_windows", pix, nbytes, len(desc), out_floats))
        return out.view(len(desc), 3 + int(self.mask), h, w), lines

    def scene_windows(self, scene, boxes, stride: int = 32):
        """RGB PIL image and integer boxes (x0, y0, x1, y1) (`scene_check`) -> (stack, lines, scene_dev): ONE (n_windows, 3 + mask, h, w)
        stack on the device with the windows of every box, bit for bit `scene_windows_host(scene, boxes, (h, w), stride, mask)`, its Line
        records, and the scene's (Hs, Ws, 3) uint8 pixels on the device (a view of the collator's device buffer: valid, in stream order,
        until the collator's next call -- what `DeviceExporter.scene` up-scales for the background).  The scene is uploaded ONCE, with the
        descriptor table and the host-resized fallback sources (`scene_plan`), from a pinned slot with one copy; one launch
        (tatt_scene_windows) reads every window out of its box's rectangle.  No boxes: the upload alone, an empty stack.  Never waits
        for the device."""
        w, h = self.lr_size
        plan = scene_plan(scene, boxes, (h, w), stride, self.mask, self._lim(line_limits))
        pix, used = scene_fill(None, plan)
        n = len(plan.desc)
        launch = self._windows("tatt_scene_windows", pix, plan.nbytes, n, plan.out_floats) if n else (
            lambda base, hbase: torch.empty(0, dtype=torch.float32, device=self.device))
        out = self._stage(used, used, lambda flat: scene_fill(flat, plan), launch)
        return out.view(n, 3 + int(self.mask), h, w), plan.lines, self._scene_dev(pix, plan)

    def _scene_dev(self, pix, plan):
        """the scene's (Hs, Ws, 3) pixels where the last upload left them: the first source behind the tables"""
        Hs, Ws = plan.arrays[0].shape[:2]
        return self._dev_buf[pix:pix + Hs * Ws * 3].view(Hs, Ws, 3)

    def quad_windows(self, scene, quads, stride: int = 32):
        """RGB PIL image and quadrilateral boxes (four integer corner points each, `quad_check`) -> (stack, lines, scene_dev): ONE
        (n_windows, 3 + mask, h, w) stack on the device with the windows of every quad's rectified crop, bit for bit
        `quad_windows_host(scene, quads, (h, w), stride, mask)`, its Line records, and the scene's (Hs, Ws, 3) uint8 pixels on the device
        (a view of the collator's device buffer, as `scene_windows` returns it).  The scene and all tables go up ONCE from a pinned slot;
        ONE tatt_warp_u8 launch writes every rectified crop into a region of the device buffer behind the upload, ONE tatt_resize_u8
        launch resizes the crops beyond `line_limits()` to (wl, h) on the device (none in the common case: no launch), ONE
        tatt_scene_windows launch reads every window out of its crop (`quad_plan`).  No quads: the upload alone, an empty stack.  Never
        waits for the device."""
        plan = quad_plan(scene, quads, self.lr_size[::-1], stride, self.mask, self._lim(line_limits), self._lim(scene_limits),
                         self._lim(quad_limits))
        return self._rectified_windows(plan)

    def _rectified_windows(self, plan):
        """a QuadPlan or PolyPlan (one layout, `quad_fill`) staged and enqueued: the rectify launch, the resize launch, the windows"""
        from . import ops
        w, h = self.lr_size
        o_warp, o_resize, o_desc, pix, used, total = quad_fill(None, plan)

        def launch(base, hbase):
            out = torch.empty(plan.out_floats, dtype=torch.float32, device=self.device)
            buf = _ptrs(base, hbase, pix)[0]
            if len(plan.warp):
                ops.call("tatt_warp_u8", buf, plan.nbytes, *_ptrs(base, hbase, o_warp), len(plan.warp), buf, plan.nbytes, ops.stream())
            if len(plan.resize):
                ops.call("tatt_resize_u8", buf, plan.nbytes, *_ptrs(base, hbase, o_resize), len(plan.resize), buf, plan.nbytes,
                         ops.stream())
            if len(plan.desc):
                ops.call("tatt_scene_windows", buf, plan.nbytes, *_ptrs(base, hbase, o_desc), len(plan.desc), ops.P(out), plan.out_floats,
                         ops.stream())
            return out
        out = self._stage(total, used, lambda flat: quad_fill(flat, plan), launch)       # (the device buffer holds the crops behind the upload)
        return out.view(len(plan.desc), 3 + int(self.mask), h, w), plan.lines, self._scene_dev(pix, plan)

    def poly_windows(self, scene, polys, stride: int = 32):
        """`quad_windows` for polygons of 2 N points (`poly_check`): curved text, straightened strip by strip -> (stack, lines,
        scene_dev), the stack bit for bit `poly_windows_host(scene, polys, (h, w), stride, mask)`.  The launches of `quad_windows`: ONE
        tatt_warp_u8 launch, with one row per STRIP, writes the strips of every polygon side by side into its crop, ONE tatt_resize_u8
        launch for the crops beyond `line_limits()` (none in the common case), ONE tatt_scene_windows launch (`poly_plan`).  No
        polygons: the upload alone, an empty stack.  Never waits for the device."""
        plan = poly_plan(scene, polys, self.lr_size[::-1], stride, self.mask, self._lim(line_limits), self._lim(scene_limits),
                         self._lim(quad_limits))
        return self._rectified_windows(plan)


# ---- image export on the device (csrc/export.hip) -----------------------------------------------------------------------------------
EXPORT_DESC = 8           # ints per descriptor row of tatt_export_images (include/tatt_hip.h)
EXPORT_RULES = {"floor": 0, "round": 1}
_EXPORT_ALIGN = 16


def _rule_code(rule):
    if rule not in EXPORT_RULES:
        raise ValueError("export rule must be 'floor' (the eval loop's astype(uint8)) or 'round' (save_image); got %r" % (rule,))
    return EXPORT_RULES[rule]


def export_limits():
    """tatt_export_limits: {'h', 'w', 'oh', 'ow', 'inter_bytes'} -- the largest source and target the device resampler takes and the most
    bytes of its horizontal pass (H * OW * 3).  An export at the native size has no limit.  A host-only entry: needs no GPU."""
    import ctypes
    from ._lib import LIB
    out = (ctypes.c_int * 5)()
    if LIB.tatt_export_limits(out) != 0:
        raise RuntimeError("tatt_export_limits failed")
    return dict(zip(("h", "w", "oh", "ow", "inter_bytes"), (int(v) for v in out)))


def quantize_u8(a, rule: str = "floor"):
    """float array -> uint8 as the reference quantises an image in [0, 1]: t = a * 255 in float32; 'floor': the eval loop
    (interfaces/super_resolution.py:1574-1587: clip to [0, 255], astype(np.uint8)); 'round': torchvision.utils.save_image
    (mul(255).add_(0.5).clamp_(0, 255).to(uint8); interfaces/base.py:590,618).  NaN becomes 0 (the reference leaves it undefined; the
    kernel, this function and tests/export_ref.py agree on 0); +-inf clips."""
    import numpy as np
    code = _rule_code(rule)
    with np.errstate(invalid="ignore", over="ignore"):
        t = np.asarray(a, dtype=np.float32) * 255
        if code:
            t = t + np.float32(0.5)
        t = np.where(np.isnan(t), np.float32(0), t)
        return np.clip(t, 0, 255).astype(np.uint8)


def _export_sizes(n, H, W, sizes):
    """None -> the native size for every item; one (w, h) -> that size for every item; else one (w, h) per item"""
    if sizes is None:
        return [(W, H)] * n
    sizes = list(sizes)
    if len(sizes) == 2 and all(isinstance(v, int) for v in sizes):
        return [tuple(sizes)] * n
    if len(sizes) != n:
        raise ValueError("%d sizes for %d images" % (len(sizes), n))
    out = [(int(w), int(h)) for w, h in sizes]
    if any(w < 1 or h < 1 for w, h in out):
        raise ValueError("export sizes must be positive (width, height) pairs")
    return out


def export_pil_batch(images, sizes=None, rule: str = "floor", c0: int = 0):
    """The host path of image export and the yardstick of `DeviceExporter`: images: a (B, C, H, W) tensor on any device -> B RGB PIL
    images of channels c0 .. c0 + 2.  Per image what the reference does (interfaces/super_resolution.py:1572-1591): `.cpu().numpy() * 255`,
    transpose, the quantisation rule (`quantize_u8`), `Image.fromarray`, and `resize(size, Image.BICUBIC)` where sizes[i] = (width, height)
    differs from the image's own size (None: no resize).  The reference resizes with cv2.INTER_CUBIC in the eval loop and with PIL in
    tripple_display; cv2 is not in this image, so this is Pillow's resize and the cv2 variant is NOT pinned (cf. `rgb_to_yuv_u8`)."""
    import numpy as np
    from PIL import Image
    B, C, H, W = images.shape
    sizes = _export_sizes(B, H, W, sizes)
    out = []
    for b in range(B):
        q = quantize_u8(np.transpose(images[b, c0:c0 + 3].detach().cpu().numpy(), (1, 2, 0)), rule)
        img = Image.fromarray(np.ascontiguousarray(q), "RGB")
        out.append(img if sizes[b] == (W, H) else img.resize(sizes[b], Image.BICUBIC))
    return out


def _export_takes(H, W, oh, ow, lim):
    if (oh, ow) == (H, W):
        return True
    if H > lim["h"] or W > lim["w"] or oh > lim["oh"] or ow > lim["ow"]:
        return False
    return W == ow or H * ow * 3 <= lim["inter_bytes"]


def export_plan(B, H, W, sizes, rule: str = "floor", limits=None, pitch=None, origin=None, c0: int = 0):
    """Host half of `DeviceExporter`, without a device: one item per image b of a (B, C, H, W) batch, sizes[b] = (width, height) its
    target.  -> (desc, resize, nbytes): desc (B, EXPORT_DESC) int32 rows [b, c0, OH, OW, rule, byte offset, row pitch, 0]; resize[b] is
    None, or (width, height) for a target beyond `limits`: that item is planned at the NATIVE size and PIL resizes it on the host after
    the copy -- exact by construction (quantisation happens before the resize on both paths), the mirror of `collate_plan`'s fallback;
    nbytes: bytes of the output the rows address.
    pitch / origin None: the items lie one after the other, rows packed (pitch 3 * OW), every item's offset 16-byte aligned.  Given (one
    int per item): the caller's canvas layout -- item b's first pixel at origin[b], its rows pitch[b] bytes apart (>= 3 * OW)."""
    import numpy as np
    lim = limits if limits is not None else export_limits()
    code = _rule_code(rule)
    sizes = _export_sizes(B, H, W, sizes)
    if (pitch is None) != (origin is None):
        raise ValueError("export_plan: pitch and origin come together")
    desc = np.zeros((B, EXPORT_DESC), np.int32)
    resize, off, end = [], 0, 0
    for b, (ow, oh) in enumerate(sizes):
        if _export_takes(H, W, oh, ow, lim):
            resize.append(None)
        else:
            resize.append((ow, oh))
            ow, oh = W, H
        p = 3 * ow if pitch is None else int(pitch[b])
        o = off if origin is None else int(origin[b])
        if p < 3 * ow or o < 0:
            raise ValueError("export_plan: item %d: pitch %d below 3 * %d or a negative origin" % (b, p, ow))
        desc[b] = (b, c0, oh, ow, code, o, p, 0)
        last = o + (oh - 1) * p + 3 * ow
        end = max(end, last)
        off = -(-last // _EXPORT_ALIGN) * _EXPORT_ALIGN
        if end >= 2 ** 31:
            raise ValueError("DeviceExporter: the batch does not fit 32-bit offsets")
    return desc, resize, end


def panel_layout(B, H, W, gap: int = 0):
    """The lr_sr_hr canvas of every sample: (height, origins) with origins[m][b] the byte offset of member m (0 LR resized to the HR size,
    1 SR, 2 HR; each H x W) of sample b; canvas b starts at b * stride (16-byte aligned), its rows 3 * W bytes apart.  gap = 0:
    make_grid(nrow=1, padding=0) of tripple_display (interfaces/base.py:580): 3 H rows.  gap > 0: the eval loop's canvas
    (interfaces/super_resolution.py:1611-1614, gap = 5): members `gap` zero rows apart and 2 * gap zero rows at the bottom, 3 H + 4 gap
    rows (its `+ 20`).  -> (height, stride, origins)"""
    height = 3 * H + 4 * gap
    stride = -(-height * 3 * W // _EXPORT_ALIGN) * _EXPORT_ALIGN
    origins = [[b * stride + m * (H + gap) * 3 * W for b in range(B)] for m in range(3)]
    return height, stride, origins


def _tables(*tables):
    """int32 tables laid behind each other, every one 16-byte aligned -> (head: the words to stage in front of the pixels, the offset of
    every table in words)"""
    import numpy as np
    offs = [0]
    for t in tables[:-1]:
        offs.append(offs[-1] + -(-t.size // 4) * 4)
    head = np.zeros(offs[-1] + tables[-1].size, np.int32)
    for o, t in zip(offs, tables):
        head[o:o + t.size] = t.reshape(-1)
    return head, offs


class _ExportSlot:
    """one pinned staging buffer of the exporter's ring: [descriptor rows | pixels]"""

    def __init__(self):
        self.host, self.held, self.event = None, False, None


class PendingExport:
    """What `DeviceExporter.__call__` / `.panels` started.  It owns one pinned slot of the exporter until `result()` / `arrays()` (which
    wait for its event only, copy the pixels out and release the slot) or `release()` (gives the slot back unread).
    `line_canvases` (of `.lines`, `.scene` and `.scene_quads`; None otherwise): (the exporter's uint8 device buffer, [(byte offset, H, W,
    row pitch)] of every blended line in it, in line order) -- where tatt_line_blend left the lines, valid until the exporter's NEXT
    call: work enqueued on the same stream before that call reads them safely (`read.LineReader.read`)."""

    def __init__(self, slot, event, pix, views, line_canvases=None):
        self._slot, self._event, self._pix, self._views, self._arrays = slot, event, pix, views, None
        self.line_canvases = line_canvases

    def arrays(self):
        """-> the (OH, OW, 3) uint8 arrays (copies: the slot is free afterwards)"""
        import numpy as np
        from PIL import Image
        if self._arrays is None:
            if self._slot is None:
                raise RuntimeError("PendingExport: released before it was read")
            self._event.synchronize()
            flat = self._slot.host.numpy()
            out = []
            for off, oh, ow, pitch, resize in self._views:
                a = np.lib.stride_tricks.as_strided(flat[self._pix + off:], (oh, ow, 3), (pitch, 3, 1)).copy()
                if resize is not None:                                  # the host fallback of export_plan
                    a = np.asarray(Image.fromarray(a, "RGB").resize(resize, Image.BICUBIC))
                out.append(a)
            self._arrays = out
            self._slot.event = None                                   # complete: nothing left to wait for
            self.release()
        return self._arrays

    def result(self):
        """-> the RGB PIL images"""
        from PIL import Image
        return [Image.fromarray(a, "RGB") for a in self.arrays()]

    def release(self):
        if self._slot is not None:
            self._slot.held = False
            self._slot = None


class DeviceExporter(_Limits):
    """`export_pil_batch` with the pixels made on the GPU: exporter(images, sizes) takes a (B, C, H, W) fp32 tensor on the device (any
    strides: the channels-last SR tensors are read as they are) and returns a `PendingExport` whose `result()` is BYTE FOR BYTE the host
    path's list of PIL images.  Per call, on the current stream: the descriptor rows go host-to-device from a pinned slot (non-blocking),
    ONE launch (tatt_export_images: quantise + PIL's bicubic resize for every image, one work-group each) fills a persistent device
    buffer, ONE non-blocking device-to-host copy brings all pixels into the pinned slot, an event is recorded.  The call never waits for
    the device; only `PendingExport.result()` / `.arrays()` do, and only for that event.
    A slot belongs to its PendingExport until that is read or `release()`d; when every slot is held the exporter adds one -- it never
    overwrites unread pixels and never blocks on the caller.  (A slot released unread is waited for before its next use.)
    The source may be a graph session's static output (`InferenceSession.run`): the launch is enqueued on the stream the next replay
    runs on, hence ordered before it -- export first, then run the next batch, no clone needed.
    Targets beyond `export_limits()` are exported at the native size and resized by PIL in `result()` (`export_plan`)."""

    def __init__(self, device="cuda", rule: str = "floor", ring: int = 3):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("tatt_amd kernels need tensors on an AMD GPU (HIP device); got %s. "
                               "There is no CPU fallback in the product path (export_pil_batch is the host path)." % self.device)
        if ring < 1:
            raise ValueError("DeviceExporter: ring must be at least 1")
        _rule_code(rule)
        self.rule, self.ring = rule, int(ring)
        self._limits = {}
        self._slots, self._i = [_ExportSlot() for _ in range(self.ring)], 0
        self._dev_buf, self._last = None, None
        self._alloc = lambda n: torch.empty(n, dtype=torch.uint8, pin_memory=True)

    def _check(self, images, c0):
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.dtype != torch.float32 or c0 < 0 or \
                images.shape[1] < c0 + 3 or images.numel() == 0:
            raise ValueError("DeviceExporter takes a 4-D fp32 tensor (B, C, H, W) with at least 3 channels from c0 = %d; got %s" % (
                c0, "%s %s" % (tuple(images.shape), images.dtype) if isinstance(images, torch.Tensor) else type(images).__name__))
        if images.device.type != "cuda":
            raise RuntimeError("tatt_amd kernels need tensors on an AMD GPU (HIP device); got %s. "
                               "There is no CPU fallback in the product path (export_pil_batch is the host path)." % images.device)

    def _slot(self, need):
        """a free slot of at least `need` bytes, now held: the next one in ring order that no PendingExport holds, else a new one"""
        n = len(self._slots)
        slot = next((self._slots[(self._i + j) % n] for j in range(n) if not self._slots[(self._i + j) % n].held), None)
        if slot is None:
            slot = _ExportSlot()
            self._slots.append(slot)
            self._i = 0
        else:
            self._i = (self._slots.index(slot) + 1) % n
        if slot.event is not None:                                     # released unread: its copy may still be in flight
            slot.event.synchronize()
            slot.event = None
        if slot.host is None or slot.host.numel() < need:
            slot.host = self._alloc(-(-need * 3 // 2 // 4096) * 4096)
        slot.held = True
        return slot

    def _enqueue(self, jobs, nbytes, views, zero=False, head=None, launch=None, canvases=None):
        """jobs: [(tensor, desc rows)], all rows addressing one output of nbytes bytes -> PendingExport.  `head` / `launch` (`lines`): the
        int32 words to stage in front of the pixels instead of the jobs' rows, and launch(device base, host base, pixel offset) instead of
        the jobs' launches.  `canvases`: [(byte offset from the pixels, H, W, pitch)] of the blended lines, for `line_canvases`."""
        import ctypes
        import numpy as np
        from . import ops
        head = np.concatenate([d.reshape(-1) for _, d in jobs]) if head is None else head
        pix = -(-head.size * 4 // _EXPORT_ALIGN) * _EXPORT_ALIGN
        cap = -(-nbytes // _EXPORT_ALIGN) * _EXPORT_ALIGN
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream()
            moved = self._last is not None and self._last[0] != stream
            if moved:
                stream.wait_event(self._last[1])                      # the one device buffer: the previous call's copy still reads it
            slot = self._slot(pix + cap)
            if self._dev_buf is None or self._dev_buf.numel() < pix + cap:
                self._dev_buf = torch.empty(slot.host.numel(), dtype=torch.uint8, device=self.device)
            elif moved:
                self._dev_buf.record_stream(stream)
            host = slot.host.numpy()
            host[:head.size * 4].view(np.int32)[:] = head
            self._dev_buf[:pix].copy_(slot.host[:pix], non_blocking=True)
            if zero:
                self._dev_buf[pix:pix + cap].zero_()
            base, hbase, r0 = self._dev_buf.data_ptr(), slot.host.data_ptr(), 0
            try:
                if launch is not None:
                    launch(base, hbase, pix)
                for t, d in jobs:
                    B, C, H, W = t.shape
                    ops.call("tatt_export_images", ops.P(t), *t.stride(), B, C, H, W, ctypes.c_void_p(base + r0 * EXPORT_DESC * 4),
                             ctypes.c_void_p(hbase + r0 * EXPORT_DESC * 4), len(d), ctypes.c_void_p(base + pix), nbytes, ops.stream())
                    r0 += len(d)
            except Exception:
                slot.held = False
                raise
            slot.host[pix:pix + cap].copy_(self._dev_buf[pix:pix + cap], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(stream)
            slot.event = ev
            self._last = (stream, ev)
            where = None if canvases is None else (self._dev_buf, [(pix + o, h, w, p) for o, h, w, p in canvases])
        return PendingExport(slot, ev, pix, views, where)

    def __call__(self, images, sizes=None, c0: int = 0) -> PendingExport:
        self._check(images, c0)
        B, _, H, W = images.shape
        desc, resize, nbytes = export_plan(B, H, W, sizes, self.rule, self._lim(export_limits), c0=c0)
        views = [(int(d[5]), int(d[2]), int(d[3]), int(d[6]), r) for d, r in zip(desc, resize)]
        return self._enqueue([(images, desc)], nbytes, views)

    def panels(self, lr, sr, hr, gap: int = 0, lr_rule: Optional[str] = None) -> PendingExport:
        """The lr_sr_hr panel of every sample (`panel_layout`): the LR image resized to the HR size on top, SR and HR below it, as one
        (3 H + 4 gap, W, 3) canvas per sample -- three launches (LR, SR, HR stacks) into one buffer, one copy back.  gap = 0 is
        make_grid(nrow=1, padding=0) of tripple_display / test_display (interfaces/base.py:565-618; there the LR image goes through
        ToPILImage, i.e. `lr_rule="floor"`, and the grid through save_image, i.e. an exporter with rule="round"); gap = 5 the eval loop's
        canvas with zero rows between (interfaces/super_resolution.py:1611-1614, rule="floor").  `lr_rule` defaults to the exporter's.
        The LR resize is Pillow's; the eval loop's cv2.resize(.., INTER_CUBIC) cannot be pinned (cv2 is not in this image), so against the
        eval loop the LR member is NOT pinned to the reference (cf. `rgb_to_yuv_u8`).  The HR size must lie within `export_limits()`."""
        for t in (lr, sr, hr):
            self._check(t, 0)
        B, _, H, W = hr.shape
        if tuple(sr.shape[2:]) != (H, W) or sr.shape[0] != B or lr.shape[0] != B:
            raise ValueError("panels: sr %s and hr %s must agree in batch and size, lr %s in batch" % (
                tuple(sr.shape), tuple(hr.shape), tuple(lr.shape)))
        if gap < 0:
            raise ValueError("panels: gap must not be negative")
        height, stride, origins = panel_layout(B, H, W, gap)
        jobs, nbytes = [], 0
        for m, (t, rule) in enumerate(((lr, lr_rule or self.rule), (sr, self.rule), (hr, self.rule))):
            desc, resize, end = export_plan(B, t.shape[2], t.shape[3], (W, H), rule, self._lim(export_limits), pitch=[3 * W] * B, origin=origins[m])
            if any(r is not None for r in resize):
                raise ValueError("panels: resizing %d x %d to %d x %d is beyond export_limits()" % (t.shape[2], t.shape[3], H, W))
            jobs.append((t, desc))
            nbytes = max(nbytes, end)
        nbytes = max(nbytes, (B - 1) * stride + height * 3 * W)
        views = [(b * stride, height, W, 3 * W, None) for b in range(B)]
        return self._enqueue(jobs, nbytes, views, zero=gap > 0)

    def _blend(self, sr_windows, lines, scale, c0):
        """sr_windows (n_windows, C, H, W) and the Line records of its lines -> ((desc, starts, nbytes) of `blend_plan`, H), the
        [(byte offset, H, W, pitch)] of the blended lines, and blend(base, hbase, o_starts, pix): the ONE tatt_line_blend launch, its
        rows at the start of the tables, its window starts `o_starts` words into them, its canvases from `pix` on.  No lines: empty
        tables, H = 0, no launch (sr_windows is not looked at)."""
        import ctypes
        import numpy as np
        from . import ops
        from .lines import BLEND_DESC
        if not lines:
            return (np.zeros((0, BLEND_DESC), np.int32), np.zeros(0, np.int32), 0, 0), [], lambda base, hbase, o_starts, pix: None
        self._check(sr_windows, c0)
        B, C, H, W = sr_windows.shape
        desc, starts, nbytes = blend_plan(lines, B, H, W, scale, self.rule, c0, self._lim(line_limits))

        def blend(base, hbase, o_starts, pix):
            ops.call("tatt_line_blend", ops.P(sr_windows), *sr_windows.stride(), B, C, H, W, *_ptrs(base, hbase, 0), len(desc),
                     *_ptrs(base, hbase, o_starts * 4), int(starts.size), ctypes.c_void_p(base + pix), nbytes, ops.stream())
        return (desc, starts, nbytes, H), [(int(d[6]), H, scale * int(d[2]), int(d[7])) for d in desc], blend

    def lines(self, sr_windows, lines, scale: int, c0: int = 0, out_sizes=None) -> PendingExport:
        """The SR windows of text lines merged into one image per line: sr_windows (n_windows, C, H, W) fp32 on the device (any strides),
        lines: the Line records of `DeviceCollator.windows`, scale = H // h -> a PendingExport whose `result()` is BYTE FOR BYTE
        `blend_windows_host(sr_windows[first:first + n], starts, wl, scale, rule, c0)` of every line, an RGB PIL image of size
        (scale * wl, H) each.  The line rows and window starts go host-to-device from a pinned slot, ONE launch (tatt_line_blend) for all
        lines, ONE non-blocking copy of all canvases back.  out_sizes[i] = (width, height): PIL resizes the finished line in `result()`
        (quantisation and blending happen before the resize on both paths)."""
        self._check(sr_windows, c0)
        lines = list(lines)
        if out_sizes is not None and len(out_sizes) != len(lines):
            raise ValueError("%d out_sizes for %d lines" % (len(out_sizes), len(lines)))
        if not lines:
            raise ValueError("DeviceExporter.lines: no lines for the %d SR windows" % sr_windows.shape[0])
        (desc, starts, nbytes, _), canvases, blend = self._blend(sr_windows, lines, scale, c0)
        views = []
        for i, (off, H, W, pitch) in enumerate(canvases):
            want = (W, H) if out_sizes is None else (int(out_sizes[i][0]), int(out_sizes[i][1]))
            views.append((off, H, W, pitch, None if want == (W, H) else want))
        head, (_, o_starts) = _tables(desc, starts)
        return self._enqueue([], nbytes, views, head=head, launch=lambda base, hbase, pix: blend(base, hbase, o_starts, pix),
                             canvases=canvases)

    def _scene_paste(self, who, scene_dev, sr_windows, lines, scale, c0, make_plan, tables, paste) -> PendingExport:
        """What `scene`, `scene_quads` and `scene_polys` (`who`) share, which is everything but their plans and their paste launches:
        the check of the scene tensor, the ONE tatt_line_blend launch of the lines, plan = make_plan((Ws, Hs), blend rows, blend bytes,
        H), the tables staged behind the blend's (tables(plan): the resize rows first), the ONE tatt_resize_u8 launch of the background,
        where the plan has `rects` the ONE tatt_resize_u8 launch of all lines into them, then per layer paste(out, nbytes, row, offs, r,
        c): the launch of the layer's c items from item r on, row(o) the (device, host) pointers of word o of the tables, offs the word
        offsets of `tables(plan)`; ONE copy back."""
        import ctypes
        from . import ops
        from .scene import RESIZE_DESC
        if not (isinstance(scene_dev, torch.Tensor) and scene_dev.dim() == 3 and scene_dev.shape[2] == 3 and
                scene_dev.dtype == torch.uint8 and scene_dev.is_contiguous() and scene_dev.device.type == "cuda"):
            raise ValueError("DeviceExporter.%s takes the contiguous (Hs, Ws, 3) uint8 scene on the device" % who)
        Hs, Ws = int(scene_dev.shape[0]), int(scene_dev.shape[1])
        (bdesc, starts, bbytes, H), canvases, blend = self._blend(sr_windows, list(lines), scale, c0)
        plan = make_plan((Ws, Hs), bdesc, bbytes, H)
        head, (_, o_starts, *offs) = _tables(bdesc, starts, *tables(plan))
        views = [(plan.canvas_off, scale * Hs, scale * Ws, plan.pitch, None)]
        nbytes, src_bytes, n = plan.nbytes, Hs * Ws * 3, len(plan.order)

        def launch(base, hbase, pix):
            out = ctypes.c_void_p(base + pix)
            blend(base, hbase, o_starts, pix)
            row = lambda o: _ptrs(base, hbase, o * 4)
            ops.call("tatt_resize_u8", ops.P(scene_dev), src_bytes, *row(offs[0]), 1, out, nbytes, ops.stream())
            if n and hasattr(plan, "rects"):                           # the line canvases lie in front of the rectangles, in the same buffer
                ops.call("tatt_resize_u8", out, max(bbytes, 1), *row(offs[0] + RESIZE_DESC), n, out, plan.canvas_off, ops.stream())
            r = 0
            for c in plan.counts:                                      # what a layer reads lies in front of the canvas
                paste(plan, out, row, offs, r, c)
                r += c
        return self._enqueue([], nbytes, views, head=head, launch=launch, canvases=canvases)

    def scene(self, scene_dev, sr_windows, lines, boxes, scale: int, feather: int = 0, c0: int = 0) -> PendingExport:
        """The finished scene: scene_dev: the (Hs, Ws, 3) uint8 scene on the device (`DeviceCollator.scene_windows`), sr_windows
        (n_windows, C, H, W) fp32 on the device: the SR windows of all boxes (None without boxes), lines: their Line records, one per box
        -> a PendingExport whose `result()` is one RGB PIL image of size (scale * Ws, scale * Hs), BYTE FOR BYTE
        `scene_compose_host(scene, boxes, [blend_windows_host(..) per box], scale, feather)`.  On the current stream: the rows of all
        launches go host-to-device from a pinned slot, ONE tatt_line_blend launch merges the windows of every box into uint8 line
        canvases that stay on the device, ONE tatt_resize_u8 launch up-scales the scene into the canvas, ONE tatt_resize_u8 launch per
        layer (`scene_layers`: boxes that do not intersect share a launch) resizes the line canvases into their rectangles, feathered
        against what the canvas holds, and ONE non-blocking copy brings the buffer into the pinned slot.  Never waits for the device."""
        from . import ops
        from .scene import RESIZE_DESC

        def paste(plan, out, row, offs, r, c):                         # the line canvases lie in front of the canvas, in the same buffer
            ops.call("tatt_resize_u8", out, plan.canvas_off, *row(offs[0] + (1 + r) * RESIZE_DESC), c, out, plan.nbytes, ops.stream())
        return self._scene_paste("scene", scene_dev, sr_windows, lines, scale, c0,
                                 lambda size, bdesc, bbytes, H: paste_plan(size, list(boxes), bdesc, bbytes, scale, H, feather,
                                                                           self._lim(scene_limits)),
                                 lambda plan: (plan.rows,), paste)

    def scene_quads(self, scene_dev, sr_windows, lines, quads, scale: int, feather: int = 0, c0: int = 0) -> PendingExport:
        """`scene` for quadrilateral boxes: scene_dev: the (Hs, Ws, 3) uint8 scene on the device (`DeviceCollator.quad_windows`),
        sr_windows (n_windows, C, H, W) fp32 on the device: the SR windows of all quads (None without quads), lines: their Line records,
        one per quad -> a PendingExport whose `result()` is one RGB PIL image of size (scale * Ws, scale * Hs), BYTE FOR BYTE
        `quad_compose_host(scene, quads, [blend_windows_host(..) per quad], scale, feather)`.  On the current stream: the rows of all
        launches go host-to-device from a pinned slot, ONE tatt_line_blend launch merges the windows of every quad into uint8 line
        canvases, ONE tatt_resize_u8 launch up-scales the scene into the canvas, ONE tatt_resize_u8 launch resizes all lines into their
        (scale * bh, scale * bw) rectangles (in the output buffer, in front of the canvas), ONE tatt_warp_u8 launch per layer
        (`quad_layers`: quads whose bounding boxes do not intersect share a launch) warps the rectangles into their quads, feathered
        against what the canvas holds, and ONE non-blocking copy brings the buffer into the pinned slot.  Never waits for the device."""
        from . import ops
        from .quads import QUAD_DESC

        def paste(plan, out, row, offs, r, c):                         # the rectangles lie in front of the canvas
            ops.call("tatt_warp_u8", out, plan.canvas_off, *row(offs[1] + r * QUAD_DESC), c, out, plan.nbytes, ops.stream())
        return self._scene_paste("scene_quads", scene_dev, sr_windows, lines, scale, c0,
                                 lambda size, bdesc, bbytes, H: quad_paste_plan(size, list(quads), bdesc, bbytes, scale, H, feather,
                                                                                self._lim(scene_limits), self._lim(quad_limits)),
                                 lambda plan: (plan.resize, plan.warp), paste)

    def scene_polys(self, scene_dev, sr_windows, lines, polys, scale: int, feather: int = 0, c0: int = 0) -> PendingExport:
        """`scene_quads` for polygons of 2 N points (curved text): scene_dev, sr_windows and lines as `DeviceCollator.poly_windows` and
        the sessions leave them, one Line per polygon -> a PendingExport whose `result()` is one RGB PIL image of size (scale * Ws,
        scale * Hs), BYTE FOR BYTE `poly_compose_host(scene, polys, [blend_windows_host(..) per polygon], scale, feather)`.  The
        launches of `scene_quads` with ONE tatt_poly_paste_u8 launch per layer (`poly_layers`) in place of its tatt_warp_u8 launches:
        every pixel of a polygon's bounding box is painted by the one strip that claims it, sampled from the whole line, feathered
        against the line's outer sides only.  Never waits for the device."""
        from . import ops
        from .polys import POLY_DESC

        def paste(plan, out, row, offs, r, c):                         # the rectangles lie in front of the canvas; ONE strip table
            ops.call("tatt_poly_paste_u8", out, plan.canvas_off, *row(offs[1] + r * POLY_DESC), c, *row(offs[2]), len(plan.strips),
                     out, plan.nbytes, ops.stream())
        return self._scene_paste("scene_polys", scene_dev, sr_windows, lines, scale, c0,
                                 lambda size, bdesc, bbytes, H: poly_paste_plan(size, list(polys), bdesc, bbytes, scale, H, feather,
                                                                                self._lim(scene_limits), self._lim(poly_limits)),
                                 lambda plan: (plan.resize, plan.items, plan.strips), paste)


from .lines import (LINE_MAX_WL, Line, blend_plan, blend_windows_host, line_limits, line_plan, line_windows_host, lines_fill,  # noqa: E402,F401
                    lines_plan, super_resolve_lines_host)
from .scene import (SCENE_MIN_SIDE, paste_plan, scene_check, scene_compose_host, scene_fill, scene_layers, scene_limits,  # noqa: E402,F401
                    scene_plan, scene_windows_host, super_resolve_scene_host)
from .quads import (QUAD_MAX_TAPER, QUAD_SHIFT, quad_bbox, quad_check, quad_compose_host, quad_fill, quad_layers,  # noqa: E402,F401
                    quad_limits, quad_matrices, quad_paste_plan, quad_plan, quad_rectify_host, quad_size, quad_windows_host,
                    super_resolve_quads_host, warp_inside_host, warp_u8_host)
from .polys import (poly_bbox, poly_check, poly_columns, poly_compose_host, poly_fill, poly_layers, poly_limits,  # noqa: E402,F401
                    poly_matrices, poly_owner_host, poly_paste_host, poly_paste_plan, poly_plan, poly_rectify_host, poly_size,
                    poly_strips, poly_windows_host, super_resolve_polys_host)
from .read import (READ_MAX, READ_QUANTUM, BeamDecoded, BeamReading, Lexicon, LexiconDecoded, LexiconReading, Reading,  # noqa: E402,F401
                   beam_limits, ctc_beam_read_host, ctc_greedy_read_host, ctc_lexicon_read_host,
                   ctc_string_logp_host, lexicon_limits, line_luma_host, read_limits, read_lines_host, read_plan, read_squeezed,
                   read_width)
from .read import WordsDecoded, WordSpan, WordsReading, ctc_words_host, ctc_words_read_host, words_limits  # noqa: E402,F401
from .read import BeamLMDecoded, BeamLMReading, CharLM, char_lm_score_host, ctc_beam_lm_read_host, lm_limits  # noqa: E402,F401
from .read import LineLexicons, ctc_line_lexicons_read_host, line_lexicons_limits  # noqa: E402,F401
