#!/usr/bin/env python3
"""Golden values of the three layer functions the reference's loss differentiates through, from the REFERENCE's own Python in fp64
(build container only; the reference is imported the way gen_golden.py imports it):

    python tests/golden/gen_layer_grad_golden.py            # writes tests/golden/layer_grads.npz

  gm_*    generate_mask(proto, coeff, box) and generate_mask(proto, coeff): seeded inputs (fp32 values), outputs and autograd gradients (fp64)
  dec_*   decode(loc, priors)
  jac_*   jaccard(a, b).diag() (the IoU term of get_DIoU, multibox_loss.py:229)
  tail_*  the tail of lincomb_mask_loss (multibox_loss.py:594-614) on a 24x40 prototype map: a 1x1 convolution and a linear layer make the
          prototypes and coefficients, the reference's generate_mask and center_size the masks and box sizes; the loss and the gradients of the
          four parameter tensors at the initial weights

The fixture holds data only.  Boxes are drawn so that the crop rectangle is the same whether its bounds are formed in fp32 or fp64 (asserted).
"""
import os
import sys

import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE)))

import gen_golden  # noqa: E402
import layer_grad_restate as R  # noqa: E402


def _boxes(n, g):
    c = torch.rand(n, 2, generator=g) * 0.6 + 0.2
    wh = torch.rand(n, 2, generator=g) * 0.5 + 0.05
    b = torch.cat((c - wh / 2, c + wh / 2), 1)
    b[1] = b[1, [2, 1, 0, 3]]                      # x1 > x2
    b[2] = torch.tensor([-0.2, 0.13, 0.43, 1.3])     # partly outside [0, 1]
    return b.float()


def _same_rect_in_fp64(boxes, h, w):
    from layers.box_utils import crop
    cm, _ = crop(torch.ones(h, w, boxes.shape[0], dtype=torch.float64), boxes.double())
    assert torch.equal(cm.permute(2, 0, 1).double(), R.crop_rect(boxes, h, w)), "a box bound lands on a pixel edge: draw other boxes"


def main():
    gen_golden.install_stubs()
    from datasets.config import set_cfg
    set_cfg("STMask_plus_resnet50_config")
    from layers.box_utils import center_size, decode, jaccard
    from layers.mask_utils import generate_mask

    out = {}
    g = torch.Generator().manual_seed(801)
    h, w, M, n = 12, 20, 8, 9
    proto, coeff, boxes = torch.relu(torch.randn(h, w, M, generator=g)), torch.randn(n, M, generator=g), _boxes(n, g)
    go = torch.randn(n, h, w, generator=g)
    _same_rect_in_fp64(boxes, h, w)
    out.update(gm_proto=proto, gm_coeff=coeff, gm_boxes=boxes, gm_grad_out=go)
    for tag, bx in (("box", boxes.double()), ("nobox", None)):
        p, c = proto.double().requires_grad_(), coeff.double().requires_grad_()
        m = generate_mask(p, c, bx)
        m.backward(go.double())
        out.update({f"gm_{tag}_out": m, f"gm_{tag}_grad_proto": p.grad, f"gm_{tag}_grad_coeff": c.grad})

    n = 33
    loc = torch.randn(n, 4, generator=g)
    pri = torch.cat((torch.rand(n, 2, generator=g), torch.rand(n, 2, generator=g) * 0.5 + 0.02), 1)
    gb = torch.randn(n, 4, generator=g)
    l64, p64 = loc.double().requires_grad_(), pri.double().requires_grad_()
    d = decode(l64, p64)
    d.backward(gb.double())
    out.update(dec_loc=loc, dec_priors=pri, dec_grad_boxes=gb, dec_out=d, dec_grad_loc=l64.grad, dec_grad_priors=p64.grad)

    n = 21
    a = _boxes(n, g)
    a[1] = a[1, [2, 1, 0, 3]]                      # (undo the swap: jaccard takes proper point-form boxes)
    a[2] = torch.tensor([0.05, 0.1, 0.4, 0.9])
    b = (a + torch.randn(n, 4, generator=g) * 0.05).float()
    b[5:9] = b[5:9] * 0.2 + torch.tensor([0.75, 0.02, 0.75, 0.02])     # disjoint pairs
    gd = torch.randn(n, generator=g)
    assert R.jaccard_ties(a.double(), b.double()) == 0
    a64, b64 = a.double().requires_grad_(), b.double().requires_grad_()
    j = jaccard(a64, b64).diag()
    j.backward(gd.double())
    assert (j == 0).sum() >= 3 and (j > 0.3).sum() >= 3
    out.update(jac_a=a, jac_b=b, jac_grad_diag=gd, jac_diag=j, jac_grad_a=a64.grad, jac_grad_b=b64.grad)

    # the loss tail, on a 24x40 prototype map with 48x80 targets
    h, w, M, C, Fdim, n = 24, 40, 8, 4, 6, 6
    x, feats, boxes = torch.randn(C, h, w, generator=g), torch.randn(n, Fdim, generator=g), _boxes(n, g).clamp(1e-5, 1)
    boxes[1] = boxes[1, [2, 1, 0, 3]]              # (the loss crops with clamped point-form boxes: x1 < x2)
    _same_rect_in_fp64(boxes, h, w)
    rect_t = R.crop_rect(boxes, 2 * h, 2 * w, padding=0)
    mask_t = ((torch.rand(n, 2 * h, 2 * w, generator=g) < 0.7).double() * rect_t)
    mask_t[:, 3:7, 5:9] = 1.0                      # some target pixels outside the crop: the BCE gradient there is the -1e12 the kernel must not touch
    weights = torch.rand(n, generator=g) + 0.5
    pw, pb = torch.randn(M, C, 1, 1, generator=g) * 0.5, torch.randn(M, generator=g) * 0.1
    cw, cb = torch.randn(M, Fdim, generator=g) * 0.5, torch.randn(M, generator=g) * 0.1
    leaves = [t.double().requires_grad_() for t in (pw, pb, cw, cb)]
    proto = torch.relu(F.conv2d(x.double()[None], leaves[0], leaves[1]))[0].permute(1, 2, 0).contiguous()
    masks = generate_mask(proto, F.linear(feats.double(), leaves[2], leaves[3]), boxes.double())
    up = F.interpolate(masks.unsqueeze(0), (2 * h, 2 * w), mode="bilinear", align_corners=False).squeeze(0)
    pre = F.binary_cross_entropy(torch.clamp(up, 0, 1), mask_t, reduction="none")
    cs = center_size(boxes.double())
    loss = torch.sum(weights.double() * (pre.sum(dim=(1, 2)) / torch.clamp(cs[:, 2] * (2 * w), min=1) / torch.clamp(cs[:, 3] * (2 * h), min=1)))
    loss.backward()
    out.update(tail_x=x, tail_feats=feats, tail_boxes=boxes, tail_mask_t=mask_t.to(torch.uint8), tail_weights=weights, tail_proto_w=pw,
               tail_proto_b=pb, tail_coef_w=cw, tail_coef_b=cb, tail_loss=loss, tail_grad_proto_w=leaves[0].grad, tail_grad_proto_b=leaves[1].grad,
               tail_grad_coef_w=leaves[2].grad, tail_grad_coef_b=leaves[3].grad)
    gen_golden.save("layer_grads.npz", **out)


if __name__ == "__main__":
    main()
