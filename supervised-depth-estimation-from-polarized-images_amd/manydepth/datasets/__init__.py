"""Datasets of the façade.

``HAMMER_Dataset`` keeps the reference's constructor signature (hammer_dataset.py:23 / indoor_dataset.py:39-57, as
called at trainer.py:276-303).  When ``data_path`` holds a HAMMER tree
(``<scene>/<modality>/{rgb,pol00,pol01,pol10,pol11,_gt,<depth_modality>,_instance}/%06d.png`` + ``intrinsics.txt``,
indoor_dataset.py:118-190, hammer_dataset.py:59-169) the items are decoded from disk with PIL (LANCZOS resize =
the reference's Image.ANTIALIAS, nearest for depth / instance masks, 16-bit depth in mm -> m).  Seeded synthetic
HAMMER-shaped items with the same keys, dtypes and shapes are served ONLY for the literal ``data_path ==
"synthetic"`` (bench.py and the tests pass it); any other path that is missing, or holds no complete frame of the
requested scenes, raises FileNotFoundError like the reference fails on a wrong ``--data_path``.

Difference to the reference by design: the four polarizer grays are handed over raw as ``("pol", 0, 0)`` uint8
[4,H,W] (order 0/45/90/135 deg = pol00, pol01, pol10, pol11, indoor_dataset.py:435-439) and DoLP/AoLP/normals are
computed on the device by K1, instead of the per-pixel ``lstsq`` in the DataLoader workers (:430-442).
Colour augmentation (indoor_dataset.py:92-106, 226-233, 300, 404-407): with probability 0.5 a training item's
``color_aug`` pyramid is the ColorJitter(brightness, contrast, saturation in [0.8, 1.2], hue in [-0.1, 0.1]) of
its ``color`` pyramid -- torchvision 0.8.2's PIL path restated on PIL.ImageEnhance (torchvision is not installed).

Opt-in (``raw_color=True`` / ``PD_DEVICE_COLOR=1``): the colour pyramids leave the workers too.  A file-backed item then
carries the decoded frame at its native size, ``("color_raw", 0, 0)`` uint8 [3,Hf,Wf], and its augmentation draw,
``"color_jitter"`` float64 [8] (``polardepth.color.pack_jitter``; zeros for a plain or an evaluation item), instead of the
eight ``color`` / ``color_aug`` tensors; Trainer.process_batch / Evaluation.predict expand them on the device
(``polardepth.color.color_pyramid``: the same successive LANCZOS resizes and ColorJitter, bit for bit).  The item draws
from ``random`` exactly as the host path does.  Default collation stacks the frames, so every frame of a batch must have
one native size -- HAMMER's do.

Opt-in (``pol_native=True`` / ``PD_POL_NATIVE=1``): the polarizer planes keep the depth of their files -- 8-bit files
(PIL mode ``L``) stay uint8, 16-bit files (``I;16``) become uint16, float files (``F``) float32 -- instead of the
``convert("L")`` that clips a 16-bit file at 255.  The worker's resize is then PIL's LANCZOS in that mode, and with
``raw_pol`` the planes travel raw and ``polardepth.resize.resize_lanczos`` gives the same bits on the device.  K1's general
kernel takes all three (polardepth/polar.py).

Opt-in (``pol_dofp=True`` / ``PD_POL_DOFP=1``): a frame's polarizer data is the sensor's interleaved division-of-focal-plane
mosaic, ONE file ``<scene>/<modality>/pol_dofp/%06d.png`` instead of ``pol00`` .. ``pol11``.  It is handed over raw at its
file depth (``L`` uint8, ``I;16*`` uint16, ``F`` float32) as ``("pol_dofp", 0, 0)`` [1,H2,W2]; the item carries no
``("pol", 0, 0)``.  ``polardepth.polar.polar_inputs`` reconstructs the planes on the device (polardepth/dofp.py).

Opt-in (``pol_cdofp=True`` / ``PD_POL_CDOFP=1``): a frame is ONE file of the COLOUR polarization sensor (a Bayer filter over the
polarizer array), ``<scene>/<modality>/pol_cdofp/%06d.png``; frames are discovered by that folder plus ``_gt`` and the depth
modality, and neither ``rgb/`` nor ``pol00`` .. ``pol11`` is needed.  The frame is handed over raw at its file depth as
``("pol_cdofp", 0, 0)`` [1,H4,W4] with the augmentation draw ``"color_jitter"`` (the draw of ``raw_color``); the item carries
no colour pyramid and no ``("pol", 0, 0)``: Trainer.process_batch / Evaluation.predict make both on the device
(polardepth/cdofp.py).  The intrinsics are scaled by the frame's own size.

Neighbouring frames (``frame_idxs`` other than ``[0]``, the photometric mode ``--depth_supervision True --pose_input True``):
for every index ``i != 0`` an item also carries ``("color", i, 0)`` float32 [3,H,W], the frame ``idx + i * offset`` resized
with LANCZOS like frame 0; ``("poses", i)`` float32 [4,4] = ``inv(inv(T_c) @ T_s)`` in fp64 from ``_pose/%06d.txt`` of frame 0
and of the neighbour (hammer_dataset.py:104-132); and ``("frame_valid", i)`` float32 scalar, 1 -- or 0 with a zero picture and
the identity pose where the neighbour or one of the pose files does not exist (the reference substitutes a dummy picture,
indoor_dataset.py:361-366).  With ``frame_idxs == [0]`` an item is, key for key and bit for bit, what it was without this.
``raw_color`` applies to frame 0 only; ``pol_cdofp`` has no ``rgb/`` folder and refuses neighbours.
``lookup_aug=True`` (opt-in; the cost-volume student's lookup frames, trainer.py:491): every neighbour also arrives as
``("color_aug", i, 0)``, the resized frame under the item's own ColorJitter draw (the frame itself when the item is not
jittered, when it is blank or when it is missing); synthetic items get the same keys.  Without the switch nothing changes.
``need_poses=False`` (opt-in; the Trainer's pose-network mode, where the poses are predicted): a neighbour is present as
soon as its picture exists, whether or not the tree has ``_pose/``; ``("poses", i)`` is then the identity unless both pose
files exist.
``neighbour_items=True`` (opt-in; ``Evaluation.test_consistency``, which runs the network on the neighbours too): every
neighbour ``i`` also arrives as ``inputs[("neighbour", i)]``, the complete single-frame item dict of the frame ``idx + i *
offset`` -- what a ``frame_idxs=[0]`` dataset with the same options returns for it (evaluation items draw nothing; a training
item's neighbours draw their own augmentation after frame 0's).  Where that frame is not one of the dataset's complete frames,
or ``("frame_valid", i)`` is 0, it is a zero item with the same keys, shapes and dtypes, and ``("frame_valid", i)`` is 0.
Default collation stacks the nested dicts.  Synthetic items get the same keys: the same scene as the camera moved by
``("poses", i)`` sees it (its depth maps are consistent with frame 0's under that pose), drawn after every other draw of the
item.  Without the switch an item is what it was, key for key and bit for bit.
"""
import glob
import os
import random

import numpy as np
import torch
from torch.utils.data import Dataset


SYNTHETIC = "synthetic"


def color_jitter_params(brightness=(0.8, 1.2), contrast=(0.8, 1.2), saturation=(0.8, 1.2), hue=(-0.1, 0.1), rng=random):
    """torchvision 0.8.2 ``ColorJitter.get_params``: one factor per property, applied in a random order."""
    ops_ = [("brightness", rng.uniform(*brightness)), ("contrast", rng.uniform(*contrast)),
            ("saturation", rng.uniform(*saturation)), ("hue", rng.uniform(*hue))]
    rng.shuffle(ops_)
    return ops_


def apply_color_jitter(img, params):
    """torchvision.transforms.functional_pil adjust_brightness / _contrast / _saturation / _hue on a PIL RGB image."""
    from PIL import Image, ImageEnhance
    for name, f in params:
        if name == "brightness":
            img = ImageEnhance.Brightness(img).enhance(f)
        elif name == "contrast":
            img = ImageEnhance.Contrast(img).enhance(f)
        elif name == "saturation":
            img = ImageEnhance.Color(img).enhance(f)
        else:
            h, s_, v = img.convert("HSV").split()
            nh = np.array(h, dtype=np.uint8)
            nh += np.uint8(int(f * 255) & 0xff)  # np.uint8(hue_factor * 255) of torchvision: truncation + uint8 wrap-around
            img = Image.merge("HSV", (Image.fromarray(nh, "L"), s_, v)).convert("RGB")
    return img


class HAMMER_Dataset(Dataset):
    def __init__(self, data_path, filenames, height, width, frame_idxs, num_scales, is_train=False, img_ext='.png',
                 offset=10, modality="polarization", supervised_depth=True, supervised_depth_only=True,
                 depth_modality="_gt", items_per_scene=8, raw_pol=None, raw_color=None, pol_native=None,
                 pol_dofp=None, pol_cdofp=None, lookup_aug=False, need_poses=True, neighbour_items=False):
        super().__init__()
        # neighbour_items: every neighbour also arrives as ("neighbour", i), its complete single-frame item (module docstring).
        # Off: an item is what it was, bit for bit.
        self.neighbour_items = bool(neighbour_items)
        # need_poses: a neighbouring frame counts as present only with both ``_pose/%06d.txt`` files (the known-pose mode).
        # False (the Trainer's pose-network mode, which predicts the poses): the picture alone decides ("frame_valid", i),
        # so sequences that ship no pose files train.  Default: an item is what it was, bit for bit.
        self.need_poses = bool(need_poses)
        # lookup_aug: the neighbouring frames also arrive as ("color_aug", i, 0), jittered with the item's own ColorJitter
        # draw -- the lookup frames of the cost-volume student (trainer.py:491).  Off: an item is what it was, bit for bit.
        self.lookup_aug = bool(lookup_aug)
        # raw_pol: hand the four polarizer images over at their native size; the Trainer resizes them on the device
        # with the Pillow-exact LANCZOS kernels before K1.  Default: $PD_DEVICE_RESIZE == "1".
        self.raw_pol = (os.environ.get("PD_DEVICE_RESIZE") == "1") if raw_pol is None else bool(raw_pol)
        # raw_color: hand the decoded RGB frame and the jitter draw over instead of the colour pyramids (module docstring).
        # Default: $PD_DEVICE_COLOR == "1".  Synthetic items are not affected.
        self.raw_color = (os.environ.get("PD_DEVICE_COLOR") == "1") if raw_color is None else bool(raw_color)
        # pol_native: keep each polarizer file's depth (module docstring).  Default: $PD_POL_NATIVE == "1".  Synthetic items
        # are not affected.
        self.pol_native = (os.environ.get("PD_POL_NATIVE") == "1") if pol_native is None else bool(pol_native)
        # pol_dofp: the polarizer data of a frame is one interleaved sensor mosaic, pol_dofp/%06d.png (module docstring).
        # Default: $PD_POL_DOFP == "1".  Synthetic items are not affected.
        self.pol_dofp = (os.environ.get("PD_POL_DOFP") == "1") if pol_dofp is None else bool(pol_dofp)
        # pol_cdofp: a frame is one raw file of the colour polarization sensor, pol_cdofp/%06d.png (module docstring).
        # Default: $PD_POL_CDOFP == "1".  Synthetic items are not affected.
        self.pol_cdofp = (os.environ.get("PD_POL_CDOFP") == "1") if pol_cdofp is None else bool(pol_cdofp)
        if self.pol_cdofp and self.pol_dofp:
            raise ValueError("HAMMER_Dataset: pol_dofp and pol_cdofp name two different sensors; choose one")
        # frame_idxs: 0 and the neighbours of the trajectory the photometric term warps into frame 0 (trainer.py:1006-1044);
        # neighbour i is frame idx + i * offset (indoor_dataset.py:319-320).  [0] = the single-frame items of the supervised mode
        self.frame_idxs = [int(i) for i in (frame_idxs if frame_idxs is not None else [0])]
        self.neighbours = [i for i in self.frame_idxs if i != 0]
        self.offset = int(offset)
        if self.neighbours and self.pol_cdofp:
            raise ValueError("HAMMER_Dataset: pol_cdofp frames have no rgb/ folder to take neighbouring colour frames from; "
                             "frame_idxs must be [0]")
        self.data_path, self.modality, self.depth_modality, self.img_ext = data_path, modality, depth_modality, img_ext
        self.height, self.width, self.num_scales = height, width, num_scales
        self.is_train = is_train
        self.synthetic = str(data_path) == SYNTHETIC
        if self.synthetic:
            self.filenames = list(filenames) if filenames else ["synthetic_scene"]
            self.frames = []
            self.items = len(self.filenames) * items_per_scene
        else:
            if not (data_path and os.path.isdir(str(data_path))):
                raise FileNotFoundError(f"HAMMER data_path {data_path!r} is not a directory (pass the literal "
                                        f"{SYNTHETIC!r} for seeded synthetic items)")
            self.filenames = list(filenames or [])
            self.frames = self._discover(self.filenames)
            if self.filenames and not self.frames:
                if self.pol_cdofp:
                    raise FileNotFoundError(f"no complete HAMMER frame (pol_cdofp, _gt, {depth_modality}) under "
                                            f"{data_path!r} for scenes {self.filenames[:3]}...")
                raise FileNotFoundError(f"no complete HAMMER frame (rgb, {'pol_dofp' if self.pol_dofp else 'pol00/01/10/11'}, _gt, "
                                        f"{depth_modality}) under "
                                        f"{data_path!r} for scenes {self.filenames[:3]}...")
            self.items = len(self.frames)
        self._complete = set(self.frames)

    # ---- real HAMMER tree -------------------------------------------------------------------------------
    def _discover(self, scenes):
        """(folder, frame_index) of every frame that has rgb, the four polarizer images (``pol_dofp``: the one mosaic), _gt
        and depth_modality; with ``pol_cdofp`` every frame that has the colour sensor file, _gt and depth_modality."""
        frames = []
        for scene in scenes or []:
            folder = os.path.join(self.data_path, scene, self.modality)
            for f in sorted(glob.glob(os.path.join(folder, "pol_cdofp" if self.pol_cdofp else "rgb", "*" + self.img_ext))):
                idx = int(os.path.basename(f).split('.')[0])
                need = [] if self.pol_cdofp else (["pol_dofp"] if self.pol_dofp else ["pol00", "pol01", "pol10", "pol11"])
                need = need + ["_gt", self.depth_modality]
                if all(os.path.isfile(os.path.join(folder, d, "{:06d}.png".format(idx))) for d in need):
                    frames.append((folder, idx))
        return frames

    def _load_item(self, folder, idx, neighbours=None):
        from PIL import Image
        neighbours = self.neighbours if neighbours is None else neighbours
        H, W = self.height, self.width
        name = "{:06d}{}".format(idx, self.img_ext)
        to_t = lambda im: torch.from_numpy(np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0)
        inputs = {}
        if self.pol_cdofp:                        # the sensor frame is picture and polarizer data at once
            frame = self._dofp_frame(os.path.join(folder, "pol_cdofp", "{:06d}.png".format(idx)), "pol_cdofp")
            full_h, full_w = frame.shape[-2:]
        else:
            color = Image.open(os.path.join(folder, "rgb", name)).convert("RGB")
            full_w, full_h = color.size
            prev = color
        do_color_aug = self.is_train and random.random() > 0.5                     # indoor_dataset.py:300
        jitter = color_jitter_params() if do_color_aug else None                   # :404-405, one draw per item
        if self.pol_cdofp:                        # demosaic, resizes, jitter and / 255 happen on the device (polardepth/cdofp.py)
            from polardepth.color import pack_jitter
            inputs[("pol_cdofp", 0, 0)] = frame
            inputs["color_jitter"] = torch.from_numpy(pack_jitter(jitter))
        elif self.raw_color:                        # resizes, jitter and / 255 happen on the device (polardepth/color.py)
            from polardepth.color import pack_jitter
            inputs[("color_raw", 0, 0)] = torch.from_numpy(np.ascontiguousarray(np.asarray(color, dtype=np.uint8).transpose(2, 0, 1)))
            inputs["color_jitter"] = torch.from_numpy(pack_jitter(jitter))
        else:
            for s in range(self.num_scales):      # successive LANCZOS resizes (indoor_dataset.py:192-215)
                prev = prev.resize((W >> s, H >> s), Image.LANCZOS)
                inputs[("color", 0, s)] = to_t(prev)
                blank = inputs[("color", 0, s)].sum() == 0                         # :222-225 blank frames stay blank
                inputs[("color_aug", 0, s)] = to_t(apply_color_jitter(prev, jitter)) if (do_color_aug and not blank) \
                    else inputs[("color", 0, s)]
        pol_paths = [os.path.join(folder, d, name) for d in ("pol00", "pol01", "pol10", "pol11")]   # 0, 45, 90, 135 degrees
        if self.pol_cdofp:
            pass                                  # the frame above carries the polarizer data too
        elif self.pol_dofp:
            inputs[("pol_dofp", 0, 0)] = self._dofp_frame(os.path.join(folder, "pol_dofp", "{:06d}.png".format(idx)))
        elif self.pol_native:
            inputs[("pol", 0, 0)] = self._native_planes(pol_paths)
        else:
            pol_imgs = [Image.open(p).convert("L") for p in pol_paths]
            planes = [np.asarray(im if self.raw_pol else im.resize((W, H), Image.LANCZOS)) for im in pol_imgs]
            inputs[("pol", 0, 0)] = torch.from_numpy(np.stack(planes).astype(np.uint8))

        def depth_of(sub):                        # 16-bit PNG in mm -> metres, nearest resize (hammer_dataset.py:135-169)
            im = Image.open(os.path.join(folder, sub, "{:06d}.png".format(idx)))
            arr = np.asarray(im.resize((W, H), Image.NEAREST)).astype(np.uint16)
            return torch.from_numpy((arr / 1000).astype(np.float32))[None]
        inputs["depth"] = depth_of(self.depth_modality)
        inputs["depth_gt"] = depth_of("_gt")
        mpath = os.path.join(folder, "_instance", "{:06d}.png".format(idx))
        if os.path.isfile(mpath):
            m = np.asarray(Image.open(mpath).convert("L").resize((W, H), Image.NEAREST))
        else:
            m = np.zeros((H, W), np.uint8)
        inputs[("mask", 0, 0)] = torch.from_numpy(m.astype(np.int32))[None]
        K0 = np.eye(4, dtype=np.float32)          # indoor_dataset.py:261-275, 379-388
        with open(os.path.join(folder, "intrinsics.txt")) as f:
            K0[:3, :3] = np.array(f.read().split(), dtype=np.float32).reshape(3, 3)
        K0[0, :] /= full_w
        K0[1, :] /= full_h
        for s in range(self.num_scales):
            K = K0.copy()
            K[0, :] *= W // (2 ** s)
            K[1, :] *= H // (2 ** s)
            inputs[("K", s)] = torch.from_numpy(K)
            inputs[("inv_K", s)] = torch.from_numpy(np.linalg.pinv(K))
        inputs["stereo_T"] = torch.eye(4)
        inputs["stereo_T"][0, 3] = -0.0498921
        single = list(inputs) if self.neighbour_items else None      # the keys of a single-frame item
        for i in neighbours:                      # indoor_dataset.py:311-366: a missing neighbour is a dummy, not an error
            inputs.update(self._neighbour(folder, idx, i, jitter))
        if self.neighbour_items:
            for i in neighbours:
                other = idx + i * self.offset
                if float(inputs[("frame_valid", i)]) != 0.0 and (folder, other) in self._complete:
                    inputs[("neighbour", i)] = self._load_item(folder, other, neighbours=())
                else:
                    inputs[("neighbour", i)] = {k: torch.zeros_like(inputs[k]) for k in single}
                    inputs[("frame_valid", i)] = torch.tensor(0.0, dtype=torch.float32)
        return inputs

    @staticmethod
    def relative_pose(pose_center, pose_side):
        """hammer_dataset.py:104-132: inv(inv(T_c) T_s) in fp64 from two ``_pose/%06d.txt`` files (16 numbers, cam-to-world):
        the motion that takes frame 0's camera coordinates to the neighbour's."""
        with open(pose_center) as f:
            T_c = np.array(f.read().split(), dtype="float").reshape(4, 4)
        with open(pose_side) as f:
            T_s = np.array(f.read().split(), dtype="float").reshape(4, 4)
        return np.linalg.inv(np.linalg.inv(T_c) @ T_s)

    def _neighbour(self, folder, idx, i, jitter=None):
        """("color", i, 0), ("poses", i), ("frame_valid", i) of the frame idx + i * offset: the colour frame resized like
        frame 0's first scale, the relative pose as float32, 1.0; zeros, the identity and 0.0 when the frame or one of the two
        pose files does not exist.  With ``lookup_aug`` also ("color_aug", i, 0): the resized frame under ``jitter``, the
        item's ColorJitter draw (None, a blank or a missing frame: the colour frame itself), as frame 0's "color_aug"."""
        from PIL import Image
        H, W = self.height, self.width
        other = idx + i * self.offset
        rgb = os.path.join(folder, "rgb", "{:06d}{}".format(other, self.img_ext))
        pc, ps = (os.path.join(folder, "_pose", "{:06d}.txt".format(k)) for k in (idx, other))
        have_poses = os.path.isfile(pc) and os.path.isfile(ps)
        if other >= 0 and os.path.isfile(rgb) and (have_poses or not self.need_poses):
            im = Image.open(rgb).convert("RGB").resize((W, H), Image.LANCZOS)
            color = torch.from_numpy(np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0)
            # need_poses=False (the poses are predicted): the picture alone makes the frame valid; ("poses", i) is then the
            # relative pose where both files happen to exist and the identity otherwise -- nothing reads it in that mode
            pose = torch.from_numpy(self.relative_pose(pc, ps).astype(np.float32)) if have_poses else torch.eye(4)
            ok = 1.0
        else:
            color, pose, ok, im = torch.zeros((3, H, W), dtype=torch.float32), torch.eye(4), 0.0, None
        out = {("color", i, 0): color, ("poses", i): pose, ("frame_valid", i): torch.tensor(ok, dtype=torch.float32)}
        if self.lookup_aug:
            out[("color_aug", i, 0)] = color
            if jitter is not None and im is not None and color.sum() != 0:
                aug = apply_color_jitter(im, jitter)
                out[("color_aug", i, 0)] = torch.from_numpy(np.asarray(aug, dtype=np.float32).transpose(2, 0, 1) / 255.0)
        return out

    @staticmethod
    def _dofp_frame(path, option="pol_dofp"):
        """The interleaved sensor mosaic, raw, at the depth it was written with: [1,H2,W2] uint8 (mode L), uint16 (I;16*) or
        float32 (F).  ``option``: the loader setting the error message names."""
        from PIL import Image
        im = Image.open(path)
        kind = "I;16" if im.mode.startswith("I;16") else im.mode
        dtypes = {"L": np.uint8, "I;16": np.uint16, "F": np.float32}
        if kind not in dtypes:
            raise ValueError(f"{path}: DoFP mosaic of mode {im.mode!r}; {option} serves L, I;16 and F")
        return torch.from_numpy(np.ascontiguousarray(np.asarray(im).astype(dtypes[kind])))[None]

    def _native_planes(self, paths):
        """The four polarizer files at the depth they were written with: [4,h,w] uint8 (mode L), uint16 (I;16, I;16L, I;16B,
        I;16N) or float32 (F), resized by PIL in that mode unless ``raw_pol`` hands them over raw."""
        from PIL import Image
        imgs = [Image.open(p) for p in paths]
        kinds = ["I;16" if im.mode.startswith("I;16") else im.mode for im in imgs]
        dtypes = {"L": np.uint8, "I;16": np.uint16, "F": np.float32}
        for p, im, kind in zip(paths, imgs, kinds):
            if kind not in dtypes:
                raise ValueError(f"{p}: polarizer image of mode {im.mode!r}; pol_native serves L, I;16 and F")
            if kind != kinds[0]:
                raise ValueError(f"{p}: polarizer image of mode {im.mode!r}, but {paths[0]} is {imgs[0].mode!r}: the four "
                                 "planes of a frame must have one mode")
        if not self.raw_pol:
            imgs = [im.resize((self.width, self.height), Image.LANCZOS) for im in imgs]
        return torch.from_numpy(np.stack([np.asarray(im).astype(dtypes[kinds[0]]) for im in imgs]))

    def __len__(self):
        return self.items

    def __getitem__(self, index):
        if self.synthetic:
            return self._synthetic_item(index)
        return self._load_item(*self.frames[index])

    # ---- synthetic items --------------------------------------------------------------------------------
    def _synthetic_item(self, index):
        rng = np.random.default_rng(index)
        inputs = self._synthetic_frame(rng, index)
        self._synthetic_neighbours(rng, inputs)
        if self.neighbour_items:                  # after every other draw: the item above is what it is without them
            for i in self.neighbours:
                inputs[("neighbour", i)] = self._synthetic_frame(rng, index, inputs[("poses", i)].numpy().astype(np.float64))
        return inputs

    def _synthetic_surface_from(self, index, T):
        """The depth surface of item ``index`` (frame 0's formula, without its holes) as the camera moved by ``T`` sees it,
        [H,W] float64: per pixel the depth d at which the point d r, taken back to frame 0, lies on the surface -- Newton
        steps on g(d) = z0(d) - surface(x0(d), y0(d)) with a difference quotient (g' stays within (0.2, 1.8) for the small
        motions drawn here)."""
        H, W = self.height, self.width
        K = np.eye(3)
        K[0, 0] = K[1, 1] = 0.65 * W; K[0, 2] = W / 2; K[1, 2] = H / 2
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        r = np.einsum("ij,jhw->ihw", np.linalg.inv(K), np.stack([xx, yy, np.ones_like(xx)]))
        Ti = np.linalg.inv(T)

        def g(d):
            X0 = np.einsum("ij,jhw->ihw", Ti[:3, :3], d * r) + Ti[:3, 3, None, None]
            x, y = K[0, 0] * X0[0] / X0[2] + K[0, 2], K[1, 1] * X0[1] / X0[2] + K[1, 2]
            return X0[2] - (1.05 + 0.7 * np.sin(x / (W / 7.0) + index) * np.cos(y / (H / 5.0)))
        d = np.full((H, W), 1.05)
        for _ in range(10):
            g0 = g(d)
            d = d - g0 * 1e-4 / (g(d + 1e-4) - g0)
        return d

    def _synthetic_frame(self, rng, index, pose=None):
        """One single-frame item from ``rng``'s next draws.  ``pose`` None: frame 0 of item ``index``; else the same scene
        from the camera moved by ``pose`` ([4,4] float64): its own pictures, mask and holes, and the depth of frame 0's
        surface as that camera sees it, so that the two depth maps are consistent under the pose."""
        H, W = self.height, self.width
        inputs = {}
        color = rng.random((3, H, W), dtype=np.float32)
        for s in range(self.num_scales):
            c = color.reshape(3, H >> s, 1 << s, W >> s, 1 << s).mean((2, 4)) if s else color
            inputs[("color", 0, s)] = torch.from_numpy(np.ascontiguousarray(c))
            inputs[("color_aug", 0, s)] = inputs[("color", 0, s)]
            K = np.eye(4, dtype=np.float32)
            K[0, 0] = K[1, 1] = 0.65 * (W >> s); K[0, 2] = (W >> s) / 2; K[1, 2] = (H >> s) / 2
            inputs[("K", s)] = torch.from_numpy(K)
            inputs[("inv_K", s)] = torch.from_numpy(np.linalg.pinv(K))
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        if pose is None:
            depth = 1.05 + 0.7 * np.sin(xx / (W / 7.0) + index) * np.cos(yy / (H / 5.0))
        else:
            depth = self._synthetic_surface_from(index, pose)
        depth[rng.random((H, W)) < 0.1] = 0
        inputs["depth"] = torch.from_numpy(depth[None].astype(np.float32))
        inputs["depth_gt"] = inputs["depth"].clone()
        inputs[("mask", 0, 0)] = torch.from_numpy((rng.integers(0, 11, (1, H, W)) * 20).astype(np.int32))
        iun = 120 + 60 * np.sin(xx / 41.0) * np.cos(yy / 37.0)
        rho = 0.02 + 0.25 * (0.5 + 0.5 * np.sin(xx / 29.0 + yy / 53.0)) ** 2
        phi = (np.pi / 2) * np.sin(xx / 61.0 - yy / 43.0)
        pol = np.stack([iun * (1 + rho * np.cos(2 * a - 2 * phi)) for a in (0, np.pi / 4, np.pi / 2, 3 * np.pi / 4)])
        pol = np.clip(np.rint(pol + rng.normal(0, 1.5, pol.shape)), 0, 255).astype(np.uint8)
        inputs[("pol", 0, 0)] = torch.from_numpy(pol)
        inputs["stereo_T"] = torch.eye(4)
        return inputs

    def _synthetic_neighbours(self, rng, inputs):
        # neighbouring frames (drawn after every draw above, so frame 0 is what it is without them): a small rigid motion and a
        # smooth colour picture -- frame 0's colour is white noise, so the term measures nothing here; it has to run and be finite
        H, W = self.height, self.width
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
        for i in self.neighbours:
            rot, t = rng.uniform(-0.01, 0.01, 3), np.array([0.03 * i, 0.0, 0.0]) + rng.uniform(-0.01, 0.01, 3)
            cx, sx = np.cos(rot[0]), np.sin(rot[0]); cy, sy = np.cos(rot[1]), np.sin(rot[1]); cz, sz = np.cos(rot[2]), np.sin(rot[2])
            T = np.eye(4)
            T[:3, :3] = (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                         @ np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))
            T[:3, 3] = t
            ph = rng.uniform(0, 2 * np.pi, 3)
            col = np.stack([0.5 + 0.3 * np.sin(xx / 11.0 + ph[c]) * np.cos(yy / 9.0 - ph[c]) + 0.15 * np.sin((xx + yy) / 17.0 + c)
                            for c in range(3)])
            inputs[("color", i, 0)] = torch.from_numpy(col.astype(np.float32))
            inputs[("poses", i)] = torch.from_numpy(T.astype(np.float32))
            inputs[("frame_valid", i)] = torch.tensor(1.0, dtype=torch.float32)
            if self.lookup_aug:                   # synthetic items are not jittered: frame 0's "color_aug" is its "color" too
                inputs[("color_aug", i, 0)] = inputs[("color", i, 0)]
        return inputs


KITTIRAWDataset = CityscapesPreprocessedDataset = KITTIOdomDataset = None   # other datasets: out of scope
