"""The cases of test_dw_strips_host.py / test_dw_strips_gpu.py: depthwise 3x3 shapes chosen by which body and which address form
of k_dw_fwd / k_dw_bwd a wave takes.  No device code.

An item is one 4-column strip (cs) of one row segment of one image, item = (b * nseg + seg) * ncs + cs, and a wave holds items
2k and 2k + 1 at any grid.  A strip is interior when its six window columns are inside the image (cs >= 1 and 4 cs + 5 <= W); a
wave takes the interior body (no column clamps, selects or guards; rows outside the image are zeros without a load) when both its
strips are interior, and the edge body otherwise: an edge strip, a second slot that wrapped into the next image or segment, an
idle slot.  Both bodies exist only in the scalar-base address form (tensor bytes < 2^32); the 64-bit form is one body.

``expect`` is what ww_dw_plan must report for the shape (waves, interior waves), worked out by hand from the rule above:

  (1, 1, 1)    one pixel: every window position but the centre is padding; top and bottom zero rows at once.  1 item.
  (1, 2, 4)    one strip that is both the left and the right edge.  1 item.
  (2, 3, 8)    two edge strips per image, no interior strip anywhere.  4 items.
  (3, 4, 12)   ncs = 3: wave (2, 3) has its second slot in the next image; 9 items, the last wave has an idle slot.  Strip 1 is
               interior (4 + 5 <= 12) but never has an interior partner: pairs (0,1) (2,0') (1',2') (0'',1'') (2'',-).
  (2, 7, 20)   ncs = 5, strips 1..3 interior: pairs (0,1) (2,3)* (4,0') (1',2')* (3',4') -- an interior pair and an
               interior + edge pair in one workgroup; 7 rows = two 3-row trips and a remainder.
  (1, 5, 21)   ncs = 6, ragged last strip with one valid column; strip 4 is interior with its right halo on the image's last
               column, and runs in the edge body beside strip 5: pairs (0,1) (2,3)* (4,5).
  (1, 23, 20)  two row segments of 12 and 11 rows: seam rows are loaded, not zero; interior pairs with hs > 0:
               seg 0: (0,1) (2,3)* (4, 0 of seg 1); seg 1: (1,2)* (3,4).
  (2, 20, 76)  the workload's image, ncs = 19 (strips 1..17 interior): 19 waves, all interior but (0,1), (18,0') and (17',18').
               At caps 1 and 3 a slot walks many items, so what a body leaves in registers meets the other body's next item."""
import torch

# (B, H, W) -> (waves, interior waves) in the scalar-base form
EXPECT = {
    (1, 1, 1): (1, 0),
    (1, 2, 4): (1, 0),
    (2, 3, 8): (2, 0),
    (3, 4, 12): (5, 0),
    (2, 7, 20): (5, 2),
    (1, 5, 21): (3, 1),
    (1, 23, 20): (5, 2),
    (2, 20, 76): (19, 16),
}
GEOMETRY = {          # (ncs, nseg, hs_len, items)
    (1, 1, 1): (1, 1, 1, 1),
    (1, 2, 4): (1, 1, 2, 1),
    (2, 3, 8): (2, 1, 3, 4),
    (3, 4, 12): (3, 1, 4, 9),
    (2, 7, 20): (5, 1, 7, 10),
    (1, 5, 21): (6, 1, 5, 6),
    (1, 23, 20): (5, 2, 12, 10),
    (2, 20, 76): (19, 1, 20, 38),
}
WORKLOAD = (2, 20, 76)
SHAPES = list(EXPECT)
WIDE_SHAPE = (2, 7, 20)             # also run with the 64-bit form forced
ACTS = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def caps(shape):
    return (1, 3) if shape == WORKLOAD else (0, 1)


def shape_id(shape):
    return "x".join(str(v) for v in shape)
