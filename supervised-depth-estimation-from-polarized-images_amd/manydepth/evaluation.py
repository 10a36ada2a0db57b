"""Evaluation (reference manydepth/evaluation.py:23-311): inference with the five trained modules
and per-material depth metrics, on the HIP forward path.  Settings mirror evaluation.py:25-48."""
import os

import numpy as np
import torch
from torch.utils.data import DataLoader

from manydepth import datasets, networks
from manydepth.utils import readlines
from polardepth import ops
from polardepth import polar as pdpolar
from polardepth import dofp as pddofp
from polardepth import cdofp as pdcdofp
from polardepth import calibration as pdcal
from polardepth import color as pdcolor
from polardepth import normals_eval
from polardepth import depth_eval
from polardepth import pointcloud
from polardepth import pose_eval
from polardepth import consistency_eval
from polardepth import polar_normals_eval
from polardepth import refine as pdrefine
from polardepth import uncertainty_eval
from polardepth import matching as pdmatching
from polardepth._records import ClassReport

_MATERIAL_GREY = {"box": 20, "bottle": 40, "can": 60, "cup": 80, "remote": 100, "teapot": 120, "cutlery": 140,
                  "glass": 160, "table": 180, "wall": 200}


def _option(value, var):
    """A constructor argument, else the environment's string (None where neither is given)."""
    return value if value is not None else os.environ.get(var)


def _switch(value, env_on):
    """A constructor argument as a bool, else what the environment says: ``env_on`` is the call's ``$PD_... == "1"``, spelled
    out there (tests/test_polar_ray_cabi.py reads it in the constructor's source)."""
    return env_on if value is None else bool(value)


_REFINE_OPTIONS = ("lam", "iters", "edge_max", "incidence_max_deg", "rho_min", "rho_max", "rounds", "uncertainty", "unc_ref",
                   "robust", "weight_min", "weight_max")


def _polar_refine_option(value, unc=None, robust=None):
    """Evaluation(polar_refine=) / $PD_POLAR_REFINE -> None (off) or the dict of options ``polar_refine`` is called with.
    ``unc`` / ``robust``: $PD_POLAR_REFINE_UNCERTAINTY ("1", or a number giving unc_ref) and $PD_POLAR_REFINE_ROBUST (c; rounds
    becomes 2 unless it is given); they fill what the options leave open and mean nothing while the refinement is off."""
    if value is None or value is False or value in ("", "0"):
        return None
    if value is True or value == "1":
        value = {}
    if isinstance(value, str):
        parts = value.split(",")
        if len(parts) != 2:
            raise ValueError(f'PD_POLAR_REFINE must be "1" or "lam,iters", got {value!r}')
        value = {"lam": float(parts[0]), "iters": int(parts[1])}
    if not isinstance(value, dict) or set(value) - set(_REFINE_OPTIONS):
        raise ValueError(f"polar_refine must be True or a dict with keys of {_REFINE_OPTIONS}, got {value!r}")
    opts = dict(value)
    if unc not in (None, "", "0") and "uncertainty" not in opts:
        opts["uncertainty"] = True
        if unc != "1":
            opts.setdefault("unc_ref", float(unc))
    if robust not in (None, "", "0") and "robust" not in opts:
        opts["robust"] = float(robust)
        opts.setdefault("rounds", 2)
    d = {"lam": 0.02, "iters": 100, "edge_max": 0.05, "incidence_max_deg": 80.0, "rounds": 1}
    pdrefine._check_solver_args(**{k: opts.get(k, v) for k, v in d.items()})
    pdrefine._check_weight_args(opts.get("unc_ref", 0.002), opts.get("robust"), opts.get("weight_min", 1 / 16),
                                opts.get("weight_max", 1.0), opts.get("rounds", 1))
    if "uncertainty" in opts and not isinstance(opts["uncertainty"], bool):
        raise ValueError(f"polar_refine's uncertainty is a switch (True / False), got {opts['uncertainty']!r}")
    return opts


class Evaluation:
    def __init__(self, load_weights_folder=None, data_path=None, height=320, width=480, batch_size=12,
                 augment_xolp=True, augment_normals=True, num_workers=0, joint_attention=None, pol_angles=None,
                 pol_layout=None, pol_demosaic=None, pol_bayer=None, pol_gains=None, pol_color_scale=None, xolp_norm=None,
                 pol_calibration=None, normals_decoder=None, pose_network=None, multi_frame=False, matching_ids=(0, -1),
                 multi_poses="files", num_depth_bins=96, depth_binning="linear", aolp_sign=None,
                 polar_ray_frame=None, uncertainty=None, uncertainty_range=None, polar_refine=None):
        """The reference hard-codes its machine's paths (evaluation.py:27-31); here they are arguments, falling back to
        $PD_EVAL_DATA_PATH / $PD_EVAL_WEIGHTS.  ``data_path="synthetic"`` serves seeded synthetic items; anything else
        must be a HAMMER tree (FileNotFoundError otherwise, like the reference on a wrong path).  ``pol_angles``: the
        calibrated polarizer angles in degrees, in the order of the planes of ("pol", 0, 0) (or $PD_POL_ANGLES="a,b,c,d",
        read here once); None = the nominal 0/45/90/135 set.  ("pol", 0, 0) may be uint8, uint16 or float32.
        ``pol_layout`` / ``pol_demosaic``: for batches that carry the interleaved sensor frame ("pol_dofp", 0, 0) instead --
        the plane each site of the 2x2 super-pixel feeds (or $PD_POL_LAYOUT="2,1,3,0") and "bilinear" | "superpixel" (or
        $PD_POL_DEMOSAIC); None = the IMX250MZR's layout, bilinear.  ``pol_angles`` then refer to the layout's planes.
        ``pol_bayer`` / ``pol_gains`` / ``pol_color_scale``: for batches that carry the COLOUR sensor frame ("pol_cdofp", 0, 0)
        -- the Bayer order (or $PD_POL_BAYER), white-balance gains r,g,b (or $PD_POL_GAINS) and the factor to the 0..255 of
        the colour picture (or $PD_POL_COLOR_SCALE; 255 / 4095 for 12-bit frames); ``pol_layout`` is shared.  None = RGGB, no
        gains, 1 for 8-bit frames.  ``xolp_norm``: the (mean, std) pair (or "mean,std") that standardises the XOLP encoder's
        input; None looks at $PD_XOLP_NORM, then at a trainer_state.pth in ``load_weights_folder`` that carries the pair the
        weights were trained with, and ends at the reference's HAMMER constants.  ``pol_calibration``: the sensor's super-pixel
        calibration (a ``polardepth.calibration.Calibration`` or the path of a saved one, or $PD_POL_CALIBRATION), applied to
        both kinds of sensor frame before their demosaic; its layout must be ``pol_layout``.  None = none.  ``normals_decoder``:
        build the `arch1++_separate_normals_dec` variant's NormalsDecoder behind the normals encoder (``predict_all``,
        ``test_normals``); None reads $PD_NORMALS_DECODER == "1", as the Trainer does.  ``pose_network``: also build the pose
        network (``pose_encoder``, ``pose``) as the Trainer's ``opt.pose_network`` mode does, and a second loader that serves
        the neighbouring frames -1 and 1 with their ground-truth poses (``test_pose``); None reads $PD_POSE_NETWORK == "1".
        Without it the object is what it was: the same models, the same draws, the same loader.

        ``multi_frame=True``: multi-frame depth inference, e.g. from a student checkpoint the reference trained
        (``encoder.pth``, ``depth.pth``, ``pose_encoder.pth``, ``pose.pth``).  Two more models, constructed AFTER every
        existing one (which therefore draw what they drew): ``encoder`` = ResnetEncoderMatching(18, False, height, width,
        adaptive_bins=True, ``num_depth_bins``, ``depth_binning``) with the bins of ``min_depth`` / ``max_depth`` until a
        checkpoint says otherwise, and ``depth`` = DepthDecoder.  ``matching_ids``: 0 and the lookup frames, as the
        reference's ``matching_ids`` (-1 .. -Ln, 1 .. Lp without gaps).  ``multi_poses``: where the sweep's poses come from --
        "files": the loader's ground-truth ``("poses", i)``; "network": the pose network's, composed link by link
        (``polardepth.matching.matching_poses``), which implies ``pose_network=True``.  A third loader
        (``multi_loader``) serves frame 0 and the lookup frames, with ``need_poses`` only for "files".  See
        ``predict_multi``, ``test_depth(source="multi")``; ``test_pose_chain`` needs the pose network only.

        ``aolp_sign``: +1 or -1, the handedness of the sensor's AoLP as ``test_polar_normals`` takes it (or
        $PD_POL_AOLP_SIGN); None = +1.  Nothing else reads it.  ``polar_ray_frame``: ``test_polar_normals`` scores in the frame
        of each pixel's viewing ray instead of the orthographic convention (``polar_normals_stats(ray_frame=True)``), for all
        its sources; None reads $PD_POLAR_RAY_FRAME == "1".  Nothing else reads it.

        ``uncertainty``: build the decoder with its uncertainty heads (``predict_all``'s "uncertainty", ``test_uncertainty``); None
        reads $PD_UNCERTAINTY == "1".  The weights folder must then hold the heads (``load_mono_model`` says so otherwise).
        ``uncertainty_range``: the (b_lo, b_hi) in metres, or "lo,hi", that turns the heads' output into a Laplace scale; None
        looks at a trainer_state.pth in ``load_weights_folder`` that carries the range the heads were trained with and ends at
        ``ops.UNCERTAINTY_RANGE``.  A convention, not a measurement.  Without ``uncertainty`` the object is what it was.

        ``polar_refine``: True, or a dict of ``polardepth.refine.polar_refine``'s options (lam, iters, edge_max,
        incidence_max_deg, rho_min, rho_max, rounds): ``predict_all`` also returns the predicted depth refined with the
        polarisation normals it disambiguates ("depth_refined", "refine_residual", "refine_touched"), and ``test_depth`` /
        ``test_normals`` take ``source="refined"``.  None reads $PD_POLAR_REFINE: "1" = the defaults (conventions, not
        measurements), "lam,iters" = those two.  It honours ``aolp_sign`` and ``polar_ray_frame``.  Without it not a bit of any
        call or report changes.  Further keys: ``uncertainty`` (True: the prior is weighted per pixel with the Laplace scale the
        decoder states, ``predict_all``'s "uncertainty"; it needs ``uncertainty=True``), ``unc_ref``, ``robust``, ``weight_min``,
        ``weight_max`` as ``polar_refine`` takes them.  $PD_POLAR_REFINE_UNCERTAINTY = "1" or a number giving ``unc_ref``, and
        $PD_POLAR_REFINE_ROBUST = c (``rounds`` becomes 2 unless it is given), fill what the options leave open."""
        self.polar_refine = _polar_refine_option(_option(polar_refine, "PD_POLAR_REFINE"),
                                                 os.environ.get("PD_POLAR_REFINE_UNCERTAINTY"), os.environ.get("PD_POLAR_REFINE_ROBUST"))
        self.uncertainty = _switch(uncertainty, os.environ.get("PD_UNCERTAINTY") == "1")
        if self.polar_refine is not None and self.polar_refine.get("uncertainty") and not self.uncertainty:
            raise ValueError('polar_refine={"uncertainty": True} weights the prior with the decoder\'s stated uncertainty: it needs '
                             "Evaluation(uncertainty=True) (or PD_UNCERTAINTY=1)")
        if isinstance(uncertainty_range, str):
            uncertainty_range = [float(x) for x in uncertainty_range.split(",")]
        if uncertainty_range is not None and not self.uncertainty:
            raise ValueError("uncertainty_range is an option of the uncertainty heads: it needs Evaluation(uncertainty=True) "
                             "(or PD_UNCERTAINTY=1)")
        self.uncertainty_range = None if uncertainty_range is None else ops.uncertainty_range(uncertainty_range)
        self.polar_ray_frame = _switch(polar_ray_frame, os.environ.get("PD_POLAR_RAY_FRAME") == "1")
        aolp_sign = _option(aolp_sign, "PD_POL_AOLP_SIGN")
        self.aolp_sign = 1 if aolp_sign is None else int(aolp_sign)
        if self.aolp_sign not in (1, -1):
            raise ValueError(f"aolp_sign must be +1 or -1, got {aolp_sign!r}")
        if multi_poses not in ("files", "network"):
            raise ValueError(f'multi_poses must be "files" or "network", got {multi_poses!r}')
        self.multi_frame, self.multi_poses = bool(multi_frame), multi_poses
        self.matching_ids = [int(i) for i in matching_ids]
        if self.multi_frame:
            pdmatching.chain_pairs(self.matching_ids)
            if multi_poses == "network":
                pose_network = True
        data_path = _option(data_path, "PD_EVAL_DATA_PATH")
        load_weights_folder = _option(load_weights_folder, "PD_EVAL_WEIGHTS")
        if data_path is None:
            raise FileNotFoundError("Evaluation needs data_path (or $PD_EVAL_DATA_PATH): a HAMMER test tree, or 'synthetic'")
        if not torch.cuda.is_available():
            raise RuntimeError("Evaluation needs the MI355X: there is no CPU fallback")
        self.height, self.width, self.batch_size = height, width, batch_size
        self.min_depth, self.max_depth, self.scales = 0.1, 2.0, [0, 1, 2, 3]
        self.augment_xolp, self.augment_normals = augment_xolp, augment_normals
        self.load_weights_folder = load_weights_folder
        self.pol_angles = pdpolar.angles_from_degrees(_option(pol_angles, "PD_POL_ANGLES"))
        pol_layout = _option(pol_layout, "PD_POL_LAYOUT")
        self.pol_dofp = pddofp.options(pol_layout, _option(pol_demosaic, "PD_POL_DEMOSAIC"))
        self.pol_cdofp = pdcdofp.options(pol_layout, _option(pol_bayer, "PD_POL_BAYER"), _option(pol_gains, "PD_POL_GAINS"),
                                         _option(pol_color_scale, "PD_POL_COLOR_SCALE"))
        self.xolp_norm = pdpolar.parse_xolp_norm(_option(xolp_norm, "PD_XOLP_NORM"))
        self.pol_calibration = pdcal.parse(_option(pol_calibration, "PD_POL_CALIBRATION"), torch.device("cuda"))
        if self.pol_calibration is not None and tuple(self.pol_calibration.layout) != tuple(self.pol_dofp[0]):
            raise ValueError(f"pol_calibration was fitted for the layout {tuple(self.pol_calibration.layout)}, pol_layout is "
                             f"{tuple(self.pol_dofp[0])}")
        # what the weights were trained with, where the arguments leave it open: one read of the Trainer's state file
        want_range = self.uncertainty and self.uncertainty_range is None
        state = {}
        if (self.xolp_norm is None or want_range) and load_weights_folder is not None:
            state_path = os.path.join(load_weights_folder, "trainer_state.pth")
            if os.path.isfile(state_path):
                state = torch.load(state_path, map_location="cpu")
        if self.xolp_norm is None:
            self.xolp_norm = pdpolar.parse_xolp_norm(state.get("xolp_norm"))
        if want_range:
            self.uncertainty_range = ops.uncertainty_range(state.get("uncertainty_range"))
        self.device = torch.device("cuda")
        self.pose_network = _switch(pose_network, os.environ.get("PD_POSE_NETWORK") == "1")
        self.models = networks.build_models(      # no pretrained weights, no dropout; the Trainer's order and draws
            False, 0.0, self.xolp_norm, self.scales, augment_normals, augment_xolp,
            attention=_switch(joint_attention, os.environ.get("PD_JOINT_ATTENTION") == "1"),
            uncertainty=self.uncertainty,
            normals_decoder=_switch(normals_decoder, os.environ.get("PD_NORMALS_DECODER") == "1"),
            pose_network=self.pose_network)
        if self.multi_frame:                      # last: the models above draw what they drew without them
            self.models["encoder"] = networks.ResnetEncoderMatching(18, False, height, width, min_depth_bin=self.min_depth,
                                                                    max_depth_bin=self.max_depth,
                                                                    num_depth_bins=num_depth_bins, adaptive_bins=True,
                                                                    depth_binning=depth_binning)
            self.models["depth"] = networks.DepthDecoder(self.models["encoder"].num_ch_enc, self.scales)
        for m in self.models.values():
            m.to(self.device).eval()
        # evaluation.py:96 reads ../splits (cwd = manydepth/); the repository root works too
        files = None
        for root in ("splits", os.path.join("..", "splits")):
            split = os.path.join(root, "HAMMER_unseen", "test_files.txt")
            if os.path.exists(split):
                files = readlines(split)
                break
        if files is None:
            if str(data_path) != datasets.SYNTHETIC:
                raise FileNotFoundError("splits/HAMMER_unseen/test_files.txt not found (evaluation.py:96)")
            files = []
        self._loader_args = (data_path, files, num_workers)
        self.test_loader = self._loader([0])
        if self.pol_calibration is not None:                  # a calibration of another frame size is refused here, not in predict
            pdcal.check_dataset(self.pol_calibration, self.test_loader.dataset, "the test loader")
        self.pose_frame_ids = [-1, 1]
        if self.pose_network:
            # a pair is scored only where the neighbour's picture and both pose files exist (need_poses=True)
            self.pose_loader = self._loader([0] + self.pose_frame_ids, supervised_depth_only=False, need_poses=True)
        self._chain_loaders = {}
        self._consistency_loaders = {}
        if self.multi_frame:
            # an absent lookup frame arrives as a zero picture with frame_valid 0 (and the identity as its pose: predict_multi
            # hands the sweep an all-zero pose instead); with "files" a frame counts only with both pose files
            self.multi_loader = self._loader([0] + self.matching_ids[1:], supervised_depth_only=False,
                                             need_poses=(multi_poses == "files"))

    def _loader(self, frame_ids, **dataset_kw):
        """The test split's items with the frames ``frame_ids``, in order, in whole batches."""
        data_path, files, num_workers = self._loader_args
        ds = datasets.HAMMER_Dataset(data_path, files, self.height, self.width, frame_ids, 4, is_train=False, **dataset_kw)
        return DataLoader(ds, self.batch_size, False, num_workers=num_workers, drop_last=True)

    def _batches(self, loader):
        """The loader's batches on the device, the nested ("neighbour", i) items of ``test_consistency`` included."""
        def to_device(d):
            return {k: to_device(v) if isinstance(v, dict) else v.to(self.device) for k, v in d.items()}
        for inputs in loader:
            yield to_device(inputs)

    def _expand(self, inputs):
        """Raw colour frames of the batch (HAMMER_Dataset(raw_color=True), colour sensor frames) -> its colour pyramids."""
        pdcolor.expand_batch(inputs, (self.height, self.width), 4, cdofp=self.pol_cdofp, calibration=self.pol_calibration)

    def _polar(self, inputs, want=("xolp", "normals")):
        """K1 on the batch (``polar_inputs``): fills ("xolp", 0, 0) and returns the nine-channel normals, if wanted."""
        return pdpolar.polar_inputs(inputs, (self.height, self.width), want, self.pol_angles, dofp=self.pol_dofp,
                                    cdofp=self.pol_cdofp, calibration=self.pol_calibration)

    def _resolve_source(self, source, allowed):
        """``source`` of a ``test_*`` method: one of ``allowed``, "auto" settled, and the option it needs switched on."""
        if source not in allowed:
            quoted = [f'"{a}"' for a in allowed]
            raise ValueError(f'source must be {", ".join(quoted[:-1])} or {quoted[-1]}, got {source!r}')
        if source == "auto":
            source = "decoder" if "normals_decoder" in self.models else "depth"
        if source == "decoder" and "normals_decoder" not in self.models:
            raise ValueError('source="decoder" needs Evaluation(normals_decoder=True) (or PD_NORMALS_DECODER=1)')
        if source == "multi" and not self.multi_frame:
            raise ValueError('source="multi" needs Evaluation(multi_frame=True)')
        if source == "refined" and self.polar_refine is None:
            raise ValueError('source="refined" needs Evaluation(polar_refine=True) (or PD_POLAR_REFINE=1)')
        return source

    def load_mono_model(self):
        if self.load_weights_folder is None:
            return
        for n, m in self.models.items():
            path = os.path.join(self.load_weights_folder, f"{n}.pth")
            # weights of a run without the variant / without the pose network / without the multi-frame student: the module
            # keeps its initialisation
            if n in ("normals_decoder", "pose_encoder", "pose", "encoder", "depth") and not os.path.isfile(path):
                continue
            sd = torch.load(path, map_location="cpu")
            if n == "encoder":
                # what the reference's save_model adds to encoder.pth (trainer.py:1607-1613), handled as its load_model
                # does (:1665-1675): the tracked depth range recomputes the bins, the size must be ours, and none of the four
                # reaches load_state_dict
                extra = {k: sd.pop(k) for k in ("height", "width", "min_depth_bin", "max_depth_bin") if k in sd}
                for k, own in (("height", self.height), ("width", self.width)):
                    if k in extra and int(extra[k]) != own:
                        raise ValueError(f"encoder.pth was trained at {k} {int(extra[k])}, this Evaluation runs at {own}")
                if extra.get("min_depth_bin") is not None and extra.get("max_depth_bin") is not None:
                    m.compute_depth_bins(float(extra["min_depth_bin"]), float(extra["max_depth_bin"]))
            if n == "mono_depth" and self.uncertainty:
                ids = {id(p) for key, conv in m.convs.items() if key[0] == "unc_conv" for p in conv.parameters()}
                heads = [k for k, p in m.named_parameters() if id(p) in ids]      # by the decoder's keys, not by index
                missing = [k for k in heads if k not in sd]
                if missing:
                    raise ValueError(f"{path} holds no unc_conv weights ({missing[0]} and {len(missing) - 1} more are missing): "
                                     "Evaluation(uncertainty=True) needs a checkpoint trained with opt.uncertainty_loss")
            m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()})

    @torch.no_grad()
    def predict(self, inputs):
        return self._forward(inputs, False)["depth"]

    @torch.no_grad()
    def predict_all(self, inputs):
        """{"depth": what ``predict`` returns, "normals_pred": the NormalsDecoder's [N,3,H,W] output} -- the latter only with
        the decoder, wired as Trainer._forward_models wires it (on the normals encoder's features).  With
        ``Evaluation(uncertainty=True)`` also "uncertainty": the Laplace scale b in metres [N,1,H,W] the scale-0 head states
        (``uncertainty_eval.scale_of`` with ``uncertainty_range``), and "uncertainty_u", the head's own output in [0, 1]."""
        return self._forward(inputs, True)

    def _depth_of(self, disp):
        """A decoder's scale-0 disparity as the depth ``predict`` returns: full resolution, clamped to the depth range."""
        return ops.disp_to_depth(disp, (self.height, self.width), self.min_depth, self.max_depth, clamp=True)

    def _forward(self, inputs, with_normals_pred):
        # HAMMER_Dataset(raw_color=True) batches; colour sensor frames are demosaicked here, for polar_inputs too
        self._expand(inputs)
        # the Trainer's hand-over: interleaved sensor frames (demosaic), un-split mosaics, raw planes of any of K1's dtypes (device LANCZOS), 612 -> 640 padding
        normals = self._polar(inputs, ("xolp", "normals") if self.augment_normals else ("xolp",))
        feats = self.models["rgb_encoder"](inputs["color_aug", 0, 0].float())
        xf = self.models["xolp_encoder"](inputs["xolp", 0, 0].float()) if self.augment_xolp else None
        nf = self.models["normals_encoder"](inputs["xolp", 0, 0].float(), normals=normals) if self.augment_normals else None
        feats = list(feats) + self.models["joint_encoder"](feats[-1], xf, nf)
        dec = self.models["mono_depth"](feats)
        out = {"depth": self._depth_of(dec[("disp", 0)])}
        if with_normals_pred and self.uncertainty:            # scale 0 is already H x W
            out["uncertainty_u"] = dec[("uncertainty", 0)].contiguous()
            out["uncertainty"] = uncertainty_eval.scale_of(out["uncertainty_u"], self.uncertainty_range)
        if with_normals_pred and "normals_decoder" in self.models:
            out["normals_pred"] = self.models["normals_decoder"](nf)
        if with_normals_pred and self.polar_refine is not None:
            pol = normals if self.augment_normals else self._polar(inputs)
            opts = dict(self.polar_refine)
            opts["uncertainty"] = out["uncertainty"] if opts.pop("uncertainty", False) else None
            ref = pdrefine.polar_refine(out["depth"], inputs[("K", 0)], pol, inputs["xolp", 0, 0], aolp_sign=self.aolp_sign,
                                        ray_frame=self.polar_ray_frame, **opts)
            out["depth_refined"], out["refine_residual"], out["refine_touched"] = ref.depth, ref.residual, ref.touched
        return out

    @torch.no_grad()
    def predict_multi(self, inputs):
        """Multi-frame depth (``multi_frame=True``): {"depth" [N,1,H,W], "lowest_cost" [N,H/4,W/4] (the disparity of the
        cheapest bin), "confidence" [N,H/4,W/4] (0/1)}.  The current frame is ("color_aug", 0, 0), the lookup frames the
        stacked ("color", i, 0) of ``matching_ids[1:]``, the intrinsics ("K", 2) / ("inv_K", 2) (the cost volume's quarter
        resolution).  The poses are ("poses", i) times ("frame_valid", i) with ``multi_poses="files"``, or the pose network's
        chain (``matching_poses`` on the ("color", i, 0) frames, the loader's ``frame_valid`` as ``present``) with
        "network": either way an absent frame reaches the sweep as an ALL-ZERO pose, which it skips -- the loader's identity
        pose would have its black picture matched.  Then the matching encoder, the decoder, and pd_disp_to_depth and the
        clamp as ``predict`` ends."""
        if not self.multi_frame:
            raise ValueError("predict_multi needs Evaluation(multi_frame=True)")
        self._expand(inputs)
        ids = self.matching_ids
        lookups = torch.stack([inputs[("color", i, 0)].float() for i in ids[1:]], 1)
        if self.multi_poses == "network":
            rel, _ = pdmatching.matching_poses(self.models["pose_encoder"], self.models["pose"],
                                               {i: inputs[("color", i, 0)] for i in ids}, ids,
                                               {i: inputs[("frame_valid", i)] for i in ids[1:]})
            poses = torch.stack([rel[i] for i in ids[1:]], 1)
        else:
            poses = torch.stack([inputs[("poses", i)].float() * inputs[("frame_valid", i)].float().view(-1, 1, 1)
                                 for i in ids[1:]], 1)
        feats, lowest_cost, confidence = self.models["encoder"](inputs[("color_aug", 0, 0)].float(), lookups, poses,
                                                                inputs[("K", 2)].float(), inputs[("inv_K", 2)].float())
        return {"depth": self._depth_of(self.models["depth"](feats)[("disp", 0)]), "lowest_cost": lowest_cost,
                "confidence": confidence}

    def test(self):
        """evaluation.py:120-288: mean over images of the 7 masked depth metrics, for the whole frame and per material
        class (instance-mask grey values :242-264).  The per-image reductions run on the device (pd_depth_metrics);
        11 x 8 numbers per batch leave the GPU instead of every depth map."""
        table = depth_eval.MaterialTable(_MATERIAL_GREY, self.min_depth, self.max_depth, self.device)
        for inputs in self._batches(self.test_loader):
            table.add(inputs["depth_gt"], self.predict(inputs), inputs[("mask", 0, 0)])
        results = table.means()
        for o, mean_errors in results.items():
            print(o, ("&{: 8.5f}  " * 7).format(*mean_errors.tolist()))
        return results

    @torch.no_grad()
    def test_normals(self, source="auto"):
        """Surface-normal accuracy per class (polardepth.normals_eval; the reference stops at depth): the angular error against
        the normals of the ground-truth depth for the whole frame, all objects and each material, one pd_normals_stats call
        per batch.  ``source``: "depth" scores the normals of the predicted depth, "decoder" the NormalsDecoder's output,
        "auto" the decoder where it exists, else depth.  Prints, and returns {class: {"per_image": [7], "pooled": [7],
        "bad": int}} with mean, median, rmse (degrees), the shares within 11.25 / 22.5 / 30 degrees and the pixel count:
        "per_image" is the mean over images of the per-image figures (this project's convention for depth; images without a
        pixel of the class do not count), "pooled" takes all pixels of all images as one set (the normals literature's).  The
        records stay on the device until the loop is over.  "refined" (``Evaluation(polar_refine=...)``) scores the normals of
        the depth refined with the polarisation normals."""
        source = self._resolve_source(source, ("auto", "depth", "decoder", "refined"))
        key = {"decoder": "normals_pred", "depth": "depth", "refined": "depth_refined"}[source]
        report = ClassReport(normals_eval.METRIC_NAMES)
        for inputs in self._batches(self.test_loader):
            out = self._forward(inputs, source != "depth")
            st = normals_eval.normals_stats(out[key], inputs["depth_gt"],
                                            inputs[("K", 0)], mask=inputs[("mask", 0, 0)], min_depth=self.min_depth,
                                            max_depth=self.max_depth)
            report.add(st, st.metrics(), st.n > 0)
        return report.finish(f"normals ({source})")

    @torch.no_grad()
    def test_polar_normals(self, source="auto", rho_min=0.05, rho_max=1.0, tilt_min_deg=5.0):
        """Does the surface agree with the polarisation that was measured (polardepth.polar_normals_eval)?  Per class -- the
        whole frame, all objects, each material -- and per batch ONE pd_polar_normals_stats call scores normals against the
        three physical candidates K1 derives from DoLP / AoLP, in two sets: "normal", the angle to the best of the six
        candidates (each and its pi flip), and "azimuth", the azimuth residual modulo pi.  It needs no ground truth and no
        pose.  ``source``: "depth" scores the normals of the predicted depth, "decoder" the NormalsDecoder's output, "auto" the
        decoder where it exists, else depth; "gt" scores the normals of the GROUND-TRUTH depth, on the pixels whose 3x3
        window is inside the depth range -- how well measurement and true geometry agree per material, the ceiling for any
        prediction.  ``xolp`` and the nine-channel normals come from ``polar_inputs`` whatever ``augment_normals`` says; the
        handedness is ``Evaluation(aolp_sign=)``.  ``rho_min`` and ``tilt_min_deg`` are conventions, not measurements
        (``polar_normals_stats``).  With ``Evaluation(polar_ray_frame=True)`` every source is scored in the frame of each
        pixel's viewing ray, and the headings say "ray frame".

        Prints, and returns {class: {"normal": r, "azimuth": r}} with r = {"per_image": [8], "pooled": [8], and the set's
        four counters by name (ints)}: mean, median, rmse (degrees), the shares within 11.25 / 22.5 / 30 degrees, the pixel
        count and the DoLP-weighted mean; "per_image" and "pooled" as in ``test_normals``.  The records stay on the device
        until the loop is over."""
        source = self._resolve_source(source, ("auto", "depth", "decoder", "gt"))
        reports = {s: ClassReport(polar_normals_eval.METRIC_NAMES) for s in ("normal", "azimuth")}
        for inputs in self._batches(self.test_loader):
            valid = None
            if source == "gt":
                pred = inputs["depth_gt"].float()
                hole = ((pred < self.min_depth) | (pred > self.max_depth) | pred.isnan()).float()
                valid = torch.nn.functional.max_pool2d(torch.nn.functional.pad(hole, (1, 1, 1, 1), mode="replicate"), 3, 1) == 0
            else:
                out = self._forward(inputs, source == "decoder")
                pred = out["normals_pred" if source == "decoder" else "depth"]
            st = polar_normals_eval.polar_normals_stats(pred, self._polar(inputs), inputs["xolp", 0, 0], K=inputs[("K", 0)],
                                                        mask=inputs[("mask", 0, 0)], valid=valid, rho_min=rho_min,
                                                        rho_max=rho_max, tilt_min_deg=tilt_min_deg, aolp_sign=self.aolp_sign,
                                                        ray_frame=self.polar_ray_frame)
            for s, report in reports.items():
                rs = getattr(st, s)
                report.add(rs, rs.metrics(), rs.n > 0)
        frame = ", ray frame" if self.polar_ray_frame else ""
        counters = lambda rs: dict(zip(rs.counter_names, rs.pooled_counters().unbind(-1)))
        sets = {s: report.finish(f"polar {s} ({source}{frame})", extras=counters) for s, report in reports.items()}
        return {name: {s: r[name] for s, r in sets.items()} for name in sets["normal"]}

    @torch.no_grad()
    def test_depth(self, median_scaling=None, source="mono"):
        """Depth accuracy per class in one pass (polardepth.depth_eval): what ``test`` reports -- and the pooled figures, the
        distribution of the absolute error and the count of unusable predictions -- for the whole frame, all objects and each
        material, one pd_depth_stats call per batch.  ``median_scaling``: None, or "numpy" / "torch" to rescale the prediction
        of every image and class by the ratio of the medians first (trainer.py:1416 / :1344), for models without metric
        supervision.  Prints, and returns {class: {"per_image": [13], "pooled": [13], "bad": int}} with abs_rel, sq_rel, rmse,
        rmse_log, a1, a2, a3, the mean and the median of |d| in millimetres, the shares of |d| below 5 / 10 / 20 mm and the
        pixel count: "per_image" is the mean over images of the per-image figures (the reference's and ``test``'s convention;
        images without a pixel of the class do not count), "pooled" takes all pixels of all images as one set.  The records
        stay on the device until the loop is over.  ``source``: "mono" scores ``predict`` over the test loader, "multi"
        (``multi_frame=True``) ``predict_multi`` over the loader that also serves the lookup frames, "refined"
        (``polar_refine=...``) ``predict_all``'s "depth_refined" -- the same scoring."""
        source = self._resolve_source(source, ("mono", "multi", "refined"))
        report = ClassReport(depth_eval.METRIC_NAMES)
        for inputs in self._batches(self.multi_loader if source == "multi" else self.test_loader):
            if source == "refined":
                depth = self.predict_all(inputs)["depth_refined"]
            else:
                depth = self.predict_multi(inputs)["depth"] if source == "multi" else self.predict(inputs)
            st = depth_eval.depth_stats(depth, inputs["depth_gt"], mask=inputs[("mask", 0, 0)], min_depth=self.min_depth,
                                        max_depth=self.max_depth, median_scaling=median_scaling)
            report.add(st, st.metrics(), st.n > 0)
        return report.finish(f"depth ({median_scaling or 'unscaled'})")

    @torch.no_grad()
    def test_uncertainty(self):
        """Does the network know where its depth is wrong (polardepth.uncertainty_eval; the reference builds the heads and
        stops there)?  Per class -- the whole frame, all objects, each material -- and per batch ONE pd_unc_stats call scores
        the scale-0 uncertainty head, read as the Laplace scale b of ``uncertainty_range``, against the error of ``predict``:
        n and bad, the mean absolute error and the mean stated scale in millimetres, the mean negative log-likelihood, the
        shares of pixels inside the central 50 % and 90 % of their stated density (0.5 and 0.9 when calibrated), and the
        sparsification figures AUSE and AURG in millimetres and relative to the mean error.  Prints, and returns {class:
        {"per_image": [10], "pooled": [10], "bad": int}} (``uncertainty_eval.METRIC_NAMES``): "per_image" is the mean over
        images of the per-image figures (images without a pixel of the class do not count), "pooled" takes all pixels of all
        images as one set, its tables added exactly.  The records stay on the device until the loop is over."""
        if not self.uncertainty:
            raise ValueError("test_uncertainty needs Evaluation(uncertainty=True) (or PD_UNCERTAINTY=1)")
        calls = []
        for inputs in self._batches(self.test_loader):
            out = self._forward(inputs, True)
            calls.append(uncertainty_eval.uncertainty_stats(out["depth"], inputs["depth_gt"], out["uncertainty_u"],
                                                            mask=inputs[("mask", 0, 0)], b_range=self.uncertainty_range,
                                                            min_depth=self.min_depth, max_depth=self.max_depth))
        if not calls:
            return {}
        # these metrics are NumPy's (the sparsification curves are drawn on the host): every image's in one array, reduced once
        per = np.concatenate([st.metrics() for st in calls], 0)              # [images, K, 10]
        valid = per[..., uncertainty_eval.METRIC_NAMES.index("n")] > 0
        with np.errstate(invalid="ignore", divide="ignore"):
            per_image = np.where(valid[..., None], per, 0.0).sum(0) / valid.sum(0)[:, None]
        report = ClassReport(uncertainty_eval.METRIC_NAMES)
        for st in calls:
            report.add(st)
        lo, hi = self.uncertainty_range
        return report.finish(f"uncertainty (b from {lo * 1e3:g} to {hi * 1e3:g} mm)", per_image=per_image)

    @torch.no_grad()
    def predict_poses(self, inputs):
        """{frame id: cam_T_cam [N,4,4]} for the neighbours of ``pose_frame_ids``: one pass of the pose network per
        neighbour on the un-jittered frame pair in temporal order, as Trainer.predict_poses runs it."""
        if not self.pose_network:
            raise ValueError("predict_poses needs Evaluation(pose_network=True) (or PD_POSE_NETWORK=1)")
        self._expand(inputs)
        cur = inputs[("color", 0, 0)].float()
        out = {}
        for f_i in self.pose_frame_ids:
            other = inputs[("color", f_i, 0)].float()
            feats = self.models["pose_encoder"](torch.cat([other, cur] if f_i < 0 else [cur, other], 1))
            out[f_i] = self.models["pose"].forward_with_matrices([feats], invert=f_i < 0)[2]
        return out

    @torch.no_grad()
    def test_pose(self):
        """Pose accuracy of the pose network (polardepth.pose_eval; the reference reports none): the predicted ``cam_T_cam``
        of every neighbour against ``("poses", i)``, one pd_pose_loss_fwd call per batch for its per-pair records, which stay
        on the device until the loop is over.  Prints, and returns {frame id: r, ..., "all": r} with r = {"pairs", "missing",
        "bad", "rot_deg": {mean, median, rmse, max of the geodesic angle in degrees}, "trans_mm": {the same of
        |t_pred - t_gt| in millimetres}, "scale_ratio_median": the median of |t_pred| / |t_gt| over the pairs with
        |t_gt| >= 1 mm}.  Pairs whose ``frame_valid`` is 0 count as ``missing``, pairs with a non-finite record as ``bad``;
        neither is averaged."""
        if not self.pose_network:
            raise ValueError("test_pose needs Evaluation(pose_network=True) (or PD_POSE_NETWORK=1)")
        ids = self.pose_frame_ids
        records, valids = [], []
        for inputs in self._batches(self.pose_loader):
            T = self.predict_poses(inputs)
            valid = torch.stack([inputs[("frame_valid", i)] for i in ids], 1).float()
            records.append(pose_eval.pair_records([T[i] for i in ids], [inputs[("poses", i)] for i in ids], valid))
            valids.append(valid)
        return self._pose_report(records, valids, ids)

    @staticmethod
    def _pose_report(records, valids, ids):
        """The per-pair records of all batches -> the printed pose table and its dict ({} without a batch)."""
        if not records:
            return {}
        results = pose_eval.metrics_from_records(torch.cat(records, 1), torch.cat(valids, 0), ids)
        print(pose_eval.format_report(results))
        return results

    @torch.no_grad()
    def test_pose_chain(self, num_links=3):
        """The drift of the composition: the pose network's chained poses 0 -> -1, .., 0 -> -num_links
        (``polardepth.matching.matching_poses`` on the un-jittered frames) against the ground-truth ``("poses", fi)``, scored
        per frame id exactly as ``test_pose`` scores single pairs (the same records and figures; its return value with the
        chain's frame ids as keys).  The loader (frames 0, -1, .., -num_links, ``need_poses=True``) is built on first use.  A
        chain counts down to its first missing frame: from there on its poses are all zero and its pairs ``missing``."""
        if not self.pose_network:
            raise ValueError("test_pose_chain needs Evaluation(pose_network=True) (or PD_POSE_NETWORK=1)")
        ids = [0] + list(range(-1, -1 - int(num_links), -1))
        pdmatching.chain_pairs(ids)
        if num_links not in self._chain_loaders:
            self._chain_loaders[num_links] = self._loader(ids, supervised_depth_only=False, need_poses=True)
        records, valids = [], []
        for inputs in self._batches(self._chain_loaders[num_links]):
            self._expand(inputs)
            present = {i: inputs[("frame_valid", i)].float() for i in ids[1:]}
            rel, _ = pdmatching.matching_poses(self.models["pose_encoder"], self.models["pose"],
                                               {i: inputs[("color", i, 0)] for i in ids}, ids, present)
            valid = torch.cumprod(torch.stack([present[i] for i in ids[1:]], 1), 1)
            records.append(pose_eval.pair_records([rel[i] for i in ids[1:]], [inputs[("poses", i)] for i in ids[1:]], valid))
            valids.append(valid)
        return self._pose_report(records, valids, ids[1:])

    @torch.no_grad()
    def test_consistency(self, ids=(-1, 1), visible="auto", per_view=False):
        """Multi-view consistency of the predicted depth per class (polardepth.consistency_eval; the reference reports none):
        ``predict`` runs on frame 0 and on every neighbour of ``ids``, and one pd_depth_consistency call per batch asks
        whether the depth maps describe the same surface under the loader's ``("poses", i)``.  The figure needs no
        ground-truth depth.  ``visible``: "auto" limits the score to the pairs the ground-truth depths of both frames say
        are mutually visible (``consistency_eval.visibility``), so that a true occlusion does not count as an inconsistency;
        None scores every pair -- occlusions then count, and the medians are the robust figures.  The loader (frames 0 and
        ``ids``, ``need_poses=True``, ``neighbour_items=True``) is built on first use; a neighbour that is missing arrives
        with ``frame_valid`` 0 and its pairs are ``absent``.  Prints the table for the whole frame, all objects and each
        material, and returns {class: {"pooled": [14] (consistency_eval.METRIC_NAMES), "n": int, "counters": int64 [8],
        "sums": float64 [4], "hist": int64 [256]}} over all pairs of the test set; with ``per_view`` also one table per
        id, from F = 1 calls, under "views": {id: {class: ...}}.  The records stay on the device until the loop is over."""
        if visible not in ("auto", None):
            raise ValueError(f'visible must be "auto" or None, got {visible!r}')
        ids = tuple(int(i) for i in ids)
        if not ids or 0 in ids or len(ids) > consistency_eval.MAX_FRAMES:
            raise ValueError(f"ids must name 1 .. {consistency_eval.MAX_FRAMES} neighbouring frames, got {ids!r}")
        if ids not in self._consistency_loaders:
            self._consistency_loaders[ids] = self._loader([0] + list(ids), supervised_depth_only=False, need_poses=True,
                                                          neighbour_items=True)
        new = lambda: ClassReport(consistency_eval.METRIC_NAMES, width=11)
        total, views = new(), {i: new() for i in ids}
        for inputs in self._batches(self._consistency_loaders[ids]):
            depth0 = self.predict(inputs)
            depths = torch.cat([self.predict(inputs[("neighbour", i)]) for i in ids], 1)
            T = torch.stack([inputs[("poses", i)] for i in ids], 1)
            valid = torch.stack([inputs[("frame_valid", i)] for i in ids], 1).float()
            K, inv_K = inputs[("K", 0)], inputs[("inv_K", 0)]
            kw = dict(mask=inputs[("mask", 0, 0)], min_depth=self.min_depth, max_depth=self.max_depth)
            vis = None
            if visible == "auto":
                gts = torch.cat([inputs[("neighbour", i)]["depth_gt"] for i in ids], 1)
                vis = consistency_eval.visibility(inputs["depth_gt"], gts, T, K, inv_K, frame_valid=valid,
                                                  min_depth=self.min_depth, max_depth=self.max_depth)
            total.add(consistency_eval.consistency(depth0, depths, T, K, inv_K, frame_valid=valid, visible=vis, want=(), **kw))
            if per_view:
                for f, i in enumerate(ids):
                    views[i].add(consistency_eval.consistency(depth0, depths[:, f:f + 1], T[:, f:f + 1], K, inv_K,
                                                              frame_valid=valid[:, f:f + 1],
                                                              visible=None if vis is None else vis[:, f:f + 1], want=(), **kw))
        # pooled figures only, and beside them the pool's own fields
        fields = lambda pool: dict(zip(("n", "counters", "sums", "hist"), pool._totals()))
        table = lambda report, title: report.finish(f"consistency ({title})", extras=fields, show_extras=False)
        how = "mutually visible pairs" if visible == "auto" else "all pairs"
        results = table(total, f"views {list(ids)}, {how}")
        if per_view and results:
            results["views"] = {i: table(views[i], f"view {i}, {how}") for i in ids}
        return results

    @torch.no_grad()
    def test_pointcloud(self, prune=True):
        """Point-cloud accuracy per class (polardepth.pointcloud; the reference opens the two clouds in a viewer,
        pointcloud/eval_pointcloud.py:256-291): the predicted and the ground-truth depth are back-projected through
        ("K", 0) at the pixels with a ground-truth depth, every point finds its exact nearest neighbour in the other cloud,
        and the distances are reported for the whole frame, all objects and each material.  Prints, and returns {class:
        {"per_image": [9], "pooled": [9], "bad": int, "unmatched": int}} with accuracy, completeness and Chamfer distance
        (mean, millimetres), the two median distances, the F-score at 5 / 10 / 20 mm and the predicted cloud's point count:
        "per_image" is the mean over images of the per-image figures (images where either cloud has no point of the class do
        not count), "pooled" takes all points of all images as one set.  ``prune=False`` takes the brute-force route of
        pd_cloud_nn: the same bits, slower.  The records stay on the device until the loop is over."""
        report = ClassReport(pointcloud.METRIC_NAMES)
        for inputs in self._batches(self.test_loader):
            depth = self.predict(inputs)
            st = pointcloud.cloud_stats(depth, inputs["depth_gt"], inputs[("K", 0)], mask=inputs[("mask", 0, 0)],
                                        min_depth=self.min_depth, max_depth=self.max_depth, prune=prune)
            report.add(st, st.metrics(), (st.acc.n > 0) & (st.comp.n > 0))
        return report.finish("pointcloud", extras=lambda t: {"bad": t.pooled_bad(), "unmatched": t.pooled_unmatched()})
