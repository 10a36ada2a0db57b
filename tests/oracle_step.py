"""Test helper: the CPU oracle's version of one training step (forward, multi-scale loss, backward) in fp32
-- what the reference's PyTorch-CPU path computes -- or with every module and input cast to fp64, the yardstick that
tells rounding noise amplified by the network from a wrong kernel (tests/test_prodsize_gpu.py, tools/grad_calibration.py).
With ``photometric`` the step carries the multi-view term of the photometric mode (oracle/reproj.py) as well, and
``multiview_batch`` is the batch on which that term measures something.  Test infrastructure only."""
import copy

import torch


def multiview_batch(B, H, W, frame_ids=(0, -1, 1), seed=3, batch_seed=5, device="cuda"):
    """A smooth, geometrically consistent batch for the photometric mode: ``synthetic.make_batch(B, H, W, frame_w=W-4,
    seed=batch_seed)`` for the polarizer planes, the masks and the pattern of invalid pixels; from
    ``synthetic.multiview_plane(B, H, W, frame_ids, seed=seed)`` the colours of every frame, the poses, ``frame_valid`` and
    the intrinsics of scale 0.  Frame 0's colour pyramid is rebuilt from the plane's picture by 2x2 averaging, and ``depth``
    / ``depth_gt`` are the plane's analytic depth, zero where make_batch's depth was zero.  (make_batch's white-noise frame
    0 cannot serve here: no depth map aligns noise with the neighbours, so the term would measure nothing.)"""
    from polardepth import synthetic
    frame_ids = tuple(int(i) for i in frame_ids)
    batch = synthetic.make_batch(B, H, W, frame_w=W - 4, device=device, seed=batch_seed)
    plane = synthetic.multiview_plane(B, H, W, frame_ids, device=device, seed=seed)
    for i in frame_ids:
        batch[("color", i, 0)] = plane[("color", i, 0)]
        if i != 0:
            batch[("poses", i)] = plane[("poses", i)]
            batch[("frame_valid", i)] = plane[("frame_valid", i)]
    batch[("K", 0)], batch[("inv_K", 0)] = plane[("K", 0)], plane[("inv_K", 0)]
    c = plane[("color", 0, 0)]
    for s in range(4):
        if s:
            c = torch.nn.functional.avg_pool2d(c, 2)
        batch[("color", 0, s)] = c
        batch[("color_aug", 0, s)] = c
    depth = torch.where(batch["depth"] == 0, torch.zeros_like(plane["depth"]), plane["depth"]).contiguous()
    batch["depth"] = depth
    batch["depth_gt"] = depth
    return batch


def _photometric_terms(cpu, inputs, depths, photometric):
    """The term of every scale of ``photometric`` (see oracle_grads) at the depth maps ``depths`` {s: [N,1,H,W]}: a list of
    oracle.reproj.photometric_term(details=True) results in the order of the scale list."""
    from oracle import reproj as orp
    ids = [int(i) for i in photometric["frame_ids"]][1:]
    valid = torch.stack([cpu[("frame_valid", i)] for i in ids], 1)
    noise, sels, coords = photometric.get("noise"), photometric.get("sels"), photometric.get("coords")
    return [orp.photometric_term(depths[s], inputs[("color", 0, 0)], [inputs[("color", i, 0)] for i in ids], inputs[("K", 0)],
                                 inputs[("inv_K", 0)], [inputs[("poses", i)] for i in ids], valid,
                                 noise=None if noise is None else noise[n], no_ssim=photometric.get("no_ssim", False),
                                 automask=photometric.get("automask", True), avg=photometric.get("avg", False),
                                 sel=None if sels is None else sels[n], coords=None if coords is None else coords[n],
                                 details=True)
            for n, s in enumerate(photometric.get("scales", range(4)))]


def oracle_term(cpu, H, W, dtype, photometric, disps=None, depths=None):
    """The photometric term alone, without the network.  ``depths`` {s: depth map}: the values {s: term_s} at those maps,
    taken as data (the forward wiring: frames, poses, intrinsics, colours, noise, options), and the selections {s: sel}
    used -- the oracle's own where ``photometric`` gives none.  ``disps`` {s: disparity}: the
    disparities are leaves, the depth maps trainer.py:538-543 makes of them; returns ({s: term_s}, {s: d sum_s'(term_s') /
    d disp_s as fp64})."""
    from oracle import losses as ol
    scales = list(photometric.get("scales", range(4)))
    inputs = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in cpu.items()}
    if disps is None:
        with torch.no_grad():
            outs = _photometric_terms(cpu, inputs, {s: depths[s].to(dtype) for s in scales}, photometric)
        return {s: float(o["loss"]) for s, o in zip(scales, outs)}, {s: o["sel"] for s, o in zip(scales, outs)}
    leaves = {s: disps[s].detach().to(dtype).requires_grad_(True) for s in scales}
    outs = _photometric_terms(cpu, inputs, {s: ol.upsample_disp_to_depth(leaves[s], H, W, 0.1, 2.0) for s in scales}, photometric)
    g = torch.autograd.grad(sum(o["loss"] for o in outs), [leaves[s] for s in scales])
    return {s: float(o["loss"].detach()) for s, o in zip(scales, outs)}, {s: gs.double() for s, gs in zip(scales, g)}


def oracle_grads(ref, cpu, H, W, dtype, photometric=None, scales=(0, 1, 2, 3)):
    """One oracle step from the modules ``ref`` and the CPU batch ``cpu``: (weight gradients of ``loss`` as fp64 tensors by
    parameter name, the loss entries as floats, the disparities).  ``scales``: the scale list of the supervised step.

    photometric: None for the supervised step, or a dict --
      frame_ids   (0, then the neighbours), as the Trainer's
      scales      the scale list of the step (default 0 1 2 3; it replaces the argument ``scales``)
      no_ssim / automask / avg    the options of the term (defaults False / True / False)
      noise       one [N,1,H,W] map per scale, added to the identity value (None without automasking)
      sels        optional, one uint8 [N,H,W] selection per scale (255 = masked) that replaces the oracle's own
      coords      optional, per scale and neighbour the pixel coordinates [N,H,W,2] of another evaluation of the warp, which
                  decide the bilinear cells in place of the oracle's own (oracle.reproj.sample_in_cells)
    -- then mean_s(term_s) joins ``loss``, term_s joins ``loss/s`` and is reported as ``reproj_loss/s`` (trainer.py:1234-1236,
    1262-1265), and a fourth value is returned: {"gdisp": {s: d sum_s'(term_s') / d disp_s}, "sels": {s: the selection used},
    "count": {s: kept pixels}}."""
    from oracle import nets as onets, losses as ol, polar as opolar
    xolp, _, _, _ = opolar.polar_forward(cpu[("pol", 0, 0)].numpy())
    models = ref if dtype == torch.float32 else {k: copy.deepcopy(m).double() for k, m in ref.items()}
    for m in models.values():
        m.train()
        for p in m.parameters():
            p.grad = None
    scales = list(scales) if photometric is None else list(photometric.get("scales", range(4)))
    color =cpu[("color_aug", 0, 0)].to(dtype)
    feats = models["rgb_encoder"](color)
    xf = models["xolp_encoder"](xolp.float().to(dtype))
    normals = opolar.get_normals(xolp.float()).float().to(dtype)           # the fp32 values the network consumes
    nf = onets.ShallowEncoder.forward(models["normals_encoder"], normals)
    feats = list(feats) + models["joint_encoder"](feats[-1], xf, nf)
    outs = dict(models["mono_depth"](feats))
    inputs = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in cpu.items()}
    for s in scales:
        outs[("depth", 0, s)] = ol.upsample_disp_to_depth(outs[("disp", s)], H, W, 0.1, 2.0)
    L = ol.compute_losses(inputs, outs, scales=scales, normals_loss_weight=0.35)
    extra = None
    if photometric is not None:
        terms = _photometric_terms(cpu, inputs, {s: outs[("depth", 0, s)] for s in scales}, photometric)
        for s, out in zip(scales, terms):
            L[f"reproj_loss/{s}"] = out["loss"]
            L[f"loss/{s}"] = L[f"loss/{s}"] + out["loss"]
        L["loss"] = L["loss"] + sum(t["loss"] for t in terms) / len(terms)
        g = torch.autograd.grad(sum(t["loss"] for t in terms), [outs[("disp", s)] for s in scales], retain_graph=True)
        extra = {"gdisp": {s: gs.detach().double() for s, gs in zip(scales, g)},
                 "sels": {s: t["sel"] for s, t in zip(scales, terms)}, "count": {s: float(t["count"]) for s, t in zip(scales, terms)}}
    L["loss"].backward()
    grads = {f"{mn}.{k}": p.grad.detach().double() for mn, m in models.items() for k, p in m.named_parameters()
             if p.grad is not None}
    res = (grads, {k: float(v.detach()) for k, v in L.items()}, {s: outs[("disp", s)].detach() for s in scales})
    return res if photometric is None else res + (extra,)
