"""The flood-extent mosaic and everything built on it: the vote canvas and its pose chain, the orthophoto under it,
frame-to-map registration, relocalisation, the merge of two mosaics, the change between them, dry-route reachability on one, and one in
metres: ground areas, map polygons and north-up rasters through a flow.georef.GroundModel.
MosaicBuilder owns all of it -- the settings, the canvases and the chain's state on the device, the per-frame report rows -- and needs
no network: only masks and the block matcher's tables.  A mosaic with its orthophoto, every frame registered against the map before it votes:

    b = MosaicBuilder((4096, 4096), ortho="centre", refine=True)
    for masks, tables, stats, frames in windows:         # device tensors: uint8 [n, H, W]; ops.block_match_modes' int32 [n, blocks, 7] and
        sources = b.check_sources(len(frames), [(f, None, "rgb24", "bt601", False) for f in frames])    # [n, 4], each frame against the one
        b.add(masks, (tables, frame_size, stats, None), sources)                                        # before it; the n decoded frames
    cls, conf, seen, totals, poses = b.report()          # the ONE read-back
    write_mosaic_part("flight.npz", b.part())            # what another builder's merge() and change_against() take

FlowPredictor (flow/predict.py) makes one from its mosaic=, ortho=, mosaic_refine= and mosaic_relocate= arguments, feeds it the masks it
hands out and keeps its reports as methods of its own; its class docstring says what every setting means.  The refusals below therefore
name FlowPredictor and its argument names.  The free functions work on "parts", the dicts part() and read_mosaic_part() return.

A builder's state is all on the device and None until the first add(): votes uint16 [classes, CH, CW], state int64 [32] (the pose
chain's), at (the origin in use), mask_size (H, W), tail int64 [12] (once a part was merged), planes = (rank, rgba) of the orthophoto,
frames (the next ordinal), merges, and the per-frame rows poses, refine_outs and relocate_outs, `chunk` frames a chunk."""
import numpy as np
import torch

from .. import ops
from .frame_rows import FrameRows

MOSAIC_STATUS = ("ok", "bridged", "lost")
REFINE_STATUS = ("corrected", "skipped", "no_fit", "out_of_bounds", "lost")
RELOCATE_STATUS = ("relocated", "not_attempted", "no_placement", "rejected_mean", "rejected_uniqueness", "fine_failed", "patch_refused", "out_of_bounds")
PART_ARRAYS = ("votes", "rank", "rgba", "state", "poses", "tail")
LINK_STATUS = ("registered", "initial", "no_fit", "out_of_bounds")


class MosaicBuilder:
    """One mosaic: size = (CH, CW), None: off -- the arguments are checked all the same, add() is never called and the reports are empty."""

    MAX_FRAMES = 1 << 31  # ordinals 0 .. 2^31 - 1: what ortho_report()'s int32 src can name

    def __init__(self, size=None, classes=5, rounds=4, tol=1.0, min_inliers=12, exclude=(1,), bridge=2, origin=None, ortho=None, refine=False, refine_search=8,
                 refine_penalty=0, refine_intra_bias=65535, refine_min_age=0, refine_every=1, relocate=False, relocate_scale=8, relocate_every=1,
                 relocate_min_overlap=0.5, relocate_exclude=2, relocate_max_mean=16, relocate_ratio=0.8, chunk=256):
        self.size = None
        self.classes = int(classes)
        if size is not None:
            if len(tuple(size)) != 2 or any(not 1 <= int(v) <= 16384 for v in size):
                raise ValueError(f"FlowPredictor: mosaic must be the canvas size (CH, CW) with 1..16384 pixels a side, got {size}")
            if not 1 <= self.classes <= 32:
                raise ValueError(f"FlowPredictor: mosaic_classes must be 1..32, got {self.classes}")
            if not 0 <= int(rounds) <= 8:
                raise ValueError(f"FlowPredictor: mosaic_rounds must be 0..8, got {rounds}")
            if not 0 <= float(tol) <= 64:
                raise ValueError(f"FlowPredictor: mosaic_tol must be 0..64 frame pixels, got {tol}")
            if not 3 <= int(min_inliers) <= 1 << 20:
                raise ValueError(f"FlowPredictor: mosaic_min_inliers must be 3..2^20, got {min_inliers}")
            ops.class_set(exclude, "mosaic_exclude", "FlowPredictor", allow_empty=True)
            if not 0 <= int(bridge) <= 64:
                raise ValueError(f"FlowPredictor: mosaic_bridge must be 0..64 frame pairs, got {bridge}")
            if origin is not None and (len(tuple(origin)) != 2 or any(abs(int(v)) > 16384 for v in origin)):
                raise ValueError(f"FlowPredictor: mosaic_origin must be (oy, ox) within 16384 pixels of the canvas corner (None: the anchor frame is "
                                 f"centred), got {origin}")
            self.size = tuple(int(v) for v in size)
        self.rounds, self.tol, self.min_inliers, self.bridge = int(rounds), float(tol), int(min_inliers), int(bridge)
        self.exclude = tuple(int(c) for c in exclude)
        self.origin = None if origin is None else tuple(int(v) for v in origin)
        if ortho is not None and ortho not in ops.ORTHO_MODES:
            raise ValueError(f"FlowPredictor: ortho must be None or one of {sorted(ops.ORTHO_MODES)}, got {ortho!r}")
        if ortho is not None and self.size is None:
            raise ValueError(f"FlowPredictor: ortho={ortho!r} needs mosaic=(CH, CW): the orthophoto is gathered with the mosaic's poses, onto its canvas")
        self.ortho = ortho
        if refine and not ortho:
            raise ValueError("FlowPredictor: mosaic_refine=True needs ortho='centre' or 'latest': a frame is registered against the orthophoto canvas")
        if not 1 <= int(refine_search) <= 32:
            raise ValueError(f"FlowPredictor: refine_search must be 1..32 pixels, got {refine_search}")
        if not 0 <= int(refine_penalty) <= 255 or not 0 <= int(refine_intra_bias) <= 65535:
            raise ValueError(f"FlowPredictor: refine_penalty must be 0..255 and refine_intra_bias 0..65535, got {refine_penalty} and {refine_intra_bias}")
        if not 0 <= int(refine_min_age) < 1 << 31:
            raise ValueError(f"FlowPredictor: refine_min_age must be 0..2^31 - 1 frames, got {refine_min_age}")
        if int(refine_every) < 1:
            raise ValueError(f"FlowPredictor: refine_every must be at least 1, got {refine_every}")
        self.refine = bool(refine)
        self.refine_search, self.refine_penalty, self.refine_intra_bias = int(refine_search), int(refine_penalty), int(refine_intra_bias)
        self.refine_min_age, self.refine_every = int(refine_min_age), int(refine_every)
        if relocate and not refine:
            raise ValueError("FlowPredictor: mosaic_relocate=True needs mosaic_refine=True: a coarse placement is committed only through the fine registration")
        if relocate_scale not in ops.RELOCATE_SCALES:
            raise ValueError(f"FlowPredictor: relocate_scale must be one of {list(ops.RELOCATE_SCALES)}, got {relocate_scale!r}")
        if int(relocate_every) < 1:
            raise ValueError(f"FlowPredictor: relocate_every must be at least 1, got {relocate_every}")
        if not 0.001 <= float(relocate_min_overlap) <= 1.0 or not 0.001 <= float(relocate_ratio) <= 1.0:
            raise ValueError(f"FlowPredictor: relocate_min_overlap and relocate_ratio must be 0.001..1, got {relocate_min_overlap} and {relocate_ratio}")
        if not 0 <= int(relocate_exclude) <= 64:
            raise ValueError(f"FlowPredictor: relocate_exclude must be 0..64 cells, got {relocate_exclude}")
        if not 0 <= int(relocate_max_mean) <= 255:
            raise ValueError(f"FlowPredictor: relocate_max_mean must be 0..255, got {relocate_max_mean}")
        self.relocate = bool(relocate)
        self.relocate_scale, self.relocate_every, self.relocate_exclude = int(relocate_scale), int(relocate_every), int(relocate_exclude)
        self.relocate_min_overlap, self.relocate_ratio = int(round(1000 * float(relocate_min_overlap))), int(round(1000 * float(relocate_ratio)))  # permille
        self.relocate_max_mean = int(relocate_max_mean)
        self.chunk = int(chunk)
        self.poses = FrameRows(((16,), torch.int64))          # the per-frame pose rows
        self.refine_outs = FrameRows(((8,), torch.int64))     # pose_correct's out rows, kept in step with poses
        self.relocate_outs = FrameRows(((8,), torch.int64))   # relocate_commit's out rows, kept in step with poses
        self.clear()

    def clear(self):
        """Drop canvases, state and report rows: the next frame anchors a new mosaic."""
        for table in (self.poses, self.refine_outs, self.relocate_outs):
            table.clear()
        self.votes = self.state = self.at = self.mask_size = self.tail = None
        self.planes, self.frames = None, 0  # (rank, rgba) [CH, CW] on the device; frames since the anchor: the next frame's ordinal
        self.merges = []                    # per merged part (link, register_mosaics' out rows, mosaic_merge's counts), on the device

    def check_sources(self, n, link_sources):
        """ortho=: the window's decoded frames, one (frame, chroma, fmt, matrix, full_range) or None per emitted frame, checked; None otherwise."""
        if not self.ortho:
            return None
        if link_sources is None or len(link_sources) != n:
            raise ValueError(f"FlowPredictor: ortho={self.ortho!r} needs link_sources with every window, one entry per frame of its n = {n} (an "
                             f"estimate-mode dataset with link_sources=True provides them), got {None if link_sources is None else len(link_sources)}; "
                             "the orthophoto is never left with a hole instead")
        if self.frames + n > self.MAX_FRAMES:  # the op takes ordinals up to 2^32 - 2; ortho_report()'s src is int32 with -1 for "none"
            raise ValueError(f"FlowPredictor: ortho= holds at most {self.MAX_FRAMES} frames per mosaic (ortho_report()'s src is int32), got "
                             f"{self.frames} + {n}; clear_report() starts a new one")
        return list(link_sources)

    def add(self, masks, link, sources=None, chunk=None):
        """A window's masks uint8 [n, H, W] into the vote canvas: one camera-motion model per frame pair from link = (tables [n, blocks, 7],
        frame size, stats [n, 4] or None, raw tables or None), the pose chain carried on in its device state, the gather, and the pose
        rows into the chunked buffers (`chunk`: default self.chunk).  ortho=: then each frame's pixels (sources: check_sources()'s list)
        into the orthophoto canvas, with that frame's pose row.  Nothing is read back."""
        masks = masks.contiguous()
        n, h, w = masks.shape
        dev, chunk = masks.device, self.chunk if chunk is None else chunk
        if self.votes is None:
            ch, cw = self.size
            self.votes = torch.zeros((self.classes, ch, cw), dtype=torch.int16, device=dev).view(torch.uint16)  # the same zero bits
            self.state = torch.zeros((32,), dtype=torch.int64, device=dev)
            self.at = self.origin if self.origin is not None else ((ch - h) // 2, (cw - w) // 2)
            self.mask_size = (h, w)
        model = ops.global_motion(link[0] if link[3] is None else link[3], link[1], (h, w), self.rounds, self.tol, self.min_inliers, mask=masks,
                                  exclude=self.exclude, pair_stats=link[2])
        if self.refine:
            poses, outs, relocs = self._refined_window(masks, model, sources)
        else:
            poses = ops.pose_chain(model, self.state, (h, w), self.size, self.at, self.bridge)
        ops.mosaic_accumulate(masks, poses, self.votes, self.at)
        for done, take, row, (rows,) in self.poses.pieces(n, chunk, dev):
            rows.copy_(poses[done:done + take])
            if self.refine:
                self.refine_outs.rows(row, take, chunk, dev)[0].copy_(outs[done:done + take])
            if self.relocate:
                self.relocate_outs.rows(row, take, chunk, dev)[0].copy_(relocs[done:done + take])
        if self.relocate:
            self.relocate_outs.frames = self.poses.frames
        if self.refine:
            self.refine_outs.frames = self.poses.frames
        elif self.ortho:
            if self.planes is None:
                self.planes = ops.ortho_canvas(self.size, dev)
            for p in range(n):
                if sources[p] is not None:
                    ops.ortho_accumulate(sources[p], poses[p], self.frames + p, (h, w), *self.planes, self.at, self.ortho)
            self.frames += n

    def _refined_window(self, masks, model, sources):
        """refine=True: the window walked frame by frame -> (poses [n, 16], pose_correct's out rows [n, 8], relocate_commit's out rows
        [n, 8] or None).  Every frame gets pose_chain with n = 1; a frame whose turn it is and whose source exists is registered against
        the orthophoto canvas -- which at that moment holds exactly the frames before it -- and its row corrected in place; with
        relocate=True the relocation sequence follows; then its pixels go into the canvas."""
        n, h, w = masks.shape
        dev, size, at = masks.device, (h, w), self.at
        if self.planes is None:
            self.planes = ops.ortho_canvas(self.size, dev)
        rank, rgba = self.planes
        poses = torch.empty((n, 16), dtype=torch.int64, device=dev)
        outs = torch.zeros((n, 8), dtype=torch.int64, device=dev)
        outs[:, 0] = 1  # not attempted
        relocs = outs.clone() if self.relocate else None
        for p in range(n):
            ordinal = self.frames + p
            poses[p:p + 1] = ops.pose_chain(model[p:p + 1], self.state, size, self.size, at, self.bridge)
            if sources[p] is None:
                continue
            if ordinal % self.refine_every == 0:
                outs[p] = self._register(sources[p], masks[p:p + 1], self.state, poses[p], ordinal)
            if self.relocate and ordinal % self.relocate_every == 0:
                relocs[p] = self._relocate(sources[p], masks[p:p + 1], poses[p], ordinal)
            ops.ortho_accumulate(sources[p], poses[p], ordinal, size, rank, rgba, at, self.ortho)
        self.frames += n
        return poses, outs, relocs

    def _register(self, source, mask, state, pose, ordinal):
        """The fine registration of one frame against the orthophoto canvas as the frame should see it under `pose`; the
        fit is folded into `state` and `pose` in place, on the device -> pose_correct's out row."""
        size, at = tuple(mask.shape[1:]), self.at
        rank, rgba = self.planes
        cur, view, valid = ops.map_view(source, pose, ordinal, size, rank, rgba, at, self.refine_min_age)
        table, stats = ops.block_match_modes(cur, view, self.refine_search, self.refine_penalty, self.refine_intra_bias, return_stats=True)
        ops.map_gate(table, valid)
        fit = ops.global_motion(table[None], size, size, self.rounds, self.tol, self.min_inliers, mask=mask, exclude=self.exclude, pair_stats=stats[None])
        return ops.pose_correct(fit, state, pose, size, self.size, at)

    def _relocate(self, source, mask, pose, ordinal):
        """One frame's relocation sequence -> relocate_commit's out row.  The chain's state and `pose` change only in
        relocate_commit's kernel, and only for a lost chain whose candidate passed the fine registration."""
        size, at, s = tuple(mask.shape[1:]), self.at, self.relocate_scale
        cl, cv = ops.map_coarse(self.planes[1], s)
        tl, tv, geom = ops.map_patch(source, self.state, size, self.size, at, s)
        found = ops.map_locate(cl, cv, tl, tv, geom, self.relocate_min_overlap, self.relocate_exclude)
        cand_state, cand_pose = ops.pose_relocate(found, self.state, size, self.size, at, s, self.relocate_max_mean, self.relocate_ratio)
        correct_out = self._register(source, mask, cand_state, cand_pose, ordinal)
        return ops.relocate_commit(cand_state, cand_pose, correct_out, self.state, pose, found, s)

    # ---- merging another mosaic into this one and the change against one
    def part(self):
        """This mosaic as a dict of DEVICE tensors (the builder's own, not copies) and plain numbers; nothing is read back."""
        if self.votes is None:
            raise ValueError("FlowPredictor: mosaic_part() needs mosaic=(CH, CW) and at least one predicted window")
        rank, rgba = self.planes if self.planes is not None else (None, None)
        tail = self.tail if self.tail is not None else self.state[:12].clone()
        return dict(votes=self.votes, rank=rank, rgba=rgba, state=self.state, poses=self.poses.flat(), tail=tail, origin=tuple(self.at),
                    mask_size=tuple(self.mask_size), frames=max(self.frames, self.poses.frames), mode=self.ortho)

    def merge(self, part, link=None, **register):
        """merge_part(self.part(), part, link, **register) with the ordinal counter and the tail carried on -> the link, on the device."""
        if self.votes is None or self.planes is None or part.get("rgba") is None:
            raise ValueError("FlowPredictor: merge_mosaic() needs mosaic= and ortho= on both sides and at least one predicted window: the registration reads both orthophotos")
        mine = self.part()
        if mine["frames"] + int(part["frames"]) > self.MAX_FRAMES:  # before anything is enqueued: a refused merge changes nothing
            raise ValueError(f"FlowPredictor: an orthophoto takes at most {self.MAX_FRAMES} frames, got {mine['frames']} + {int(part['frames'])} with the part")
        link, outs, counts = merge_part(mine, part, link, **register)
        self.frames, self.tail = mine["frames"], mine["tail"]
        self.merges.append((link, outs, counts))
        return link

    def change_against(self, part, **kw):
        """mosaic_change(self.part(), part, **kw): neither mosaic is changed; nothing is read back."""
        return mosaic_change(self.part(), part, **kw)

    def access(self, **kw):
        """mosaic_access(self, **kw): dry-route reachability on this mosaic; the mosaic is not changed."""
        return mosaic_access(self, **kw)

    def ground(self, model, **kw):
        """mosaic_ground(self, model, **kw): this mosaic in metres and as north-up rasters; the mosaic is not changed."""
        return mosaic_ground(self, model, **kw)

    def merge_report(self):
        """(links int64 numpy [parts, 16], per part the out rows [rows, 8], counts [parts, 8]) of the parts merged.  The ONE read-back."""
        if not self.merges:
            return np.zeros((0, 16), np.int64), [], np.zeros((0, 8), np.int64)
        flat = torch.cat([t.reshape(-1) for m in self.merges for t in m]).cpu().numpy()
        links, outs, counts, at = [], [], [], 0
        for _, o, _ in self.merges:
            rows = int(o.shape[0])
            links.append(flat[at:at + 16]), outs.append(flat[at + 16:at + 16 + 8 * rows].reshape(rows, 8)), counts.append(flat[at + 16 + 8 * rows:at + 24 + 8 * rows])
            at += 24 + 8 * rows
        return np.stack(links), outs, np.stack(counts)

    def _out_rows(self, on, table, name):
        if not on:
            raise ValueError(f"FlowPredictor: {name}_report() needs mosaic_{name}=True")
        return table.flat().cpu().numpy() if table.chunks else np.zeros((0, 8), np.int64)

    def relocate_report(self):
        """relocate=True: int64 numpy [frames, 8], relocate_commit's out row of every frame, in the order of report()'s poses.  The ONE read-back."""
        return self._out_rows(self.relocate, self.relocate_outs, "relocate")

    def refine_report(self):
        """refine=True: int64 numpy [frames, 8], pose_correct's out row of every frame, in the order of report()'s poses.  The ONE read-back."""
        return self._out_rows(self.refine, self.refine_outs, "refine")

    def ortho_report(self, palette=ops.FLOOD_PALETTE, alpha=None, edge=(), fill=(0, 0, 0), overlay=True):
        """ortho=: (image uint8 numpy [CH, CW, 3], src int32 [CH, CW], covered); mosaic_resolve (overlay=True), ortho_compose and the ONE
        read-back run here."""
        if not self.ortho:
            raise ValueError("FlowPredictor: ortho_report() needs ortho='centre' or 'latest'")
        ch, cw = self.size
        if self.planes is None:
            image = np.empty((ch, cw, 3), np.uint8)
            image[:] = np.array(fill, np.uint8)
            return image, np.full((ch, cw), -1, np.int32), 0
        rank, rgba = self.planes
        cls = ops.mosaic_resolve(self.votes)[0] if overlay else None
        image = ops.ortho_compose(rgba, cls, palette, alpha, fill, edge)
        src = torch.where(rank == -1, rank, rank & 0xFFFFFFFF).to(torch.int32).cpu().numpy()
        return image.cpu().numpy(), src, int((src >= 0).sum())

    def report(self):
        """(cls uint8 numpy [CH, CW], conf uint8, seen int32, totals int64 [K, 2], poses int64 [frames, 16]); the resolve pass and the ONE
        read-back run here."""
        if self.votes is None:
            ch, cw = self.size or (0, 0)
            return (np.full((ch, cw), 255, np.uint8), np.zeros((ch, cw), np.uint8), np.zeros((ch, cw), np.int32), np.zeros((self.classes, 2), np.int64),
                    np.zeros((0, 16), np.int64))
        cls, conf, seen, totals = ops.mosaic_resolve(self.votes)
        return cls.cpu().numpy(), conf.cpu().numpy(), seen.cpu().numpy(), totals.cpu().numpy(), self.poses.flat().cpu().numpy()


def write_relocate_csv(path, frame_ids, report):
    """FlowPredictor.relocate_report()'s int64 [frames, 8] as a CSV, one row per frame: frame id, status, the shift in canvas pixels, the
    best placement's summed absolute difference and cells, the runner-up's, and the eligible placements."""
    report = np.asarray(report)
    if report.ndim != 2 or report.shape[1] != 8 or len(frame_ids) != report.shape[0]:
        raise ValueError(f"write_relocate_csv: report must be [frames, 8] with one frame id per row, got {report.shape} and {len(frame_ids)} ids")
    with open(path, "w", newline="") as f:
        f.write("frame,status,shift_x,shift_y,sad,cells,sad2,cells2,eligible\n")
        for fid, row in zip(frame_ids, report.tolist()):
            f.write(",".join([str(int(fid)), RELOCATE_STATUS[row[0]] if 0 <= row[0] < len(RELOCATE_STATUS) else "patch_refused"] + [str(v) for v in row[1:]]) + "\n")


def _compose_q20(a, b):
    """mosaic_defs.h's compose (b first) on int64 device tensors [6]: the merged tail, without a read-back."""
    half = 1 << 19
    lin = [((a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + half) >> 20) + (a[3 * r + 2] if c == 2 else 0) for r in range(2) for c in range(3)]
    return torch.stack(lin)


def _placed_on_one_mask_size(what, a, b, place):
    """merge_part's and mosaic_change's (`what`) common ground: masks of one size -> `place`, with b's seen box where it names no b_box."""
    if tuple(int(v) for v in a["mask_size"]) != tuple(int(v) for v in b["mask_size"]):
        raise ValueError(f"{what}: both mosaics must be of masks of one size (a canvas pixel is a mask pixel of the anchor frame), got "
                         f"{tuple(a['mask_size'])} and {tuple(b['mask_size'])}")
    if place is not None and "b_box" not in place and b.get("box") is not None:
        return dict(place, b_box=tuple(int(v) for v in b["box"]))
    return place


def merge_part(mine, part, link=None, **register):
    """Register the mosaic `part` against the mosaic `mine` (mosaic_part()'s or read_mosaic_part()'s dicts, both with an orthophoto, on
    one device) and fold it in: ops.register_mosaics, then ops.mosaic_merge with mine's frame count as the ordinal offset.  mine's votes,
    rank and rgba are updated in place, mine["frames"] grows by the part's and mine["tail"] becomes compose(b_to_a, part's tail) where
    the link registered (decided on the device).  link: default mine's tail with status 1.  -> (link, outs, counts), device tensors."""
    dev = mine["votes"].device
    if (mine.get("mode") or None) != (part.get("mode") or None) or mine.get("mode") not in ops.ORTHO_MODES:
        raise ValueError(f"merge_part: both mosaics need an orthophoto of ONE mode (a rank word's key means the distance from the optical axis in 'centre' "
                         f"and the ordinal in 'latest'), got {mine.get('mode')!r} and {part.get('mode')!r}")
    place = _placed_on_one_mask_size("merge_part", mine, part, register.get("place"))
    if link is None:
        link = torch.cat([mine["tail"], torch.tensor([ops.LINK_INITIAL, 0, 0, 0], dtype=torch.int64, device=dev)])
    if place is not None:
        register["place"] = place
    at, other = tuple(int(v) for v in mine["origin"]), tuple(int(v) for v in part["origin"])
    link, outs = ops.register_mosaics((mine["rgba"], at), (part["rgba"], other), link, **register)
    counts = ops.mosaic_merge(mine["votes"], at, part["votes"], other, link, (mine["rank"], mine["rgba"]), (part["rank"], part["rgba"]), int(mine["frames"]),
                              mine["mode"])
    moved = torch.cat([_compose_q20(link[0:6], part["tail"][0:6]), _compose_q20(part["tail"][6:12], link[6:12])])
    mine["tail"] = torch.where(link[12] == ops.LINK_REGISTERED, moved, mine["tail"])
    mine["frames"] = int(mine["frames"]) + int(part["frames"])
    return link, outs, counts


def part_seen_box(poses, mask_size, canvas_size, origin):
    """(y0, x0, y1, x1): the canvas box that holds every frame that voted, from the pose rows on the host (frame_clipped's corners, clipped
    to the canvas); the whole canvas if none did."""
    (h, w), (ch, cw), (oy, ox) = mask_size, canvas_size, origin
    xs, ys = [], []
    for row in np.asarray(poses).tolist():
        if row[12] not in (0, 1):
            continue
        for x, y in ((0, 0), (w, 0), (0, h), (w, h)):
            xs.append(row[0] * x + row[1] * y + row[2] + ox * (1 << 20)), ys.append(row[3] * x + row[4] * y + row[5] + oy * (1 << 20))
    if not xs:
        return 0, 0, ch, cw
    y0, x0 = max(0, min(ys) >> 20), max(0, min(xs) >> 20)
    y1, x1 = min(ch, (max(ys) + (1 << 20) - 1) >> 20), min(cw, (max(xs) + (1 << 20) - 1) >> 20)
    return (y0, x0, y1, x1) if y0 < y1 and x0 < x1 else (0, 0, ch, cw)


def mosaic_part_arrays(part):
    """FlowPredictor.mosaic_part()'s dict as the numpy arrays of a part file (the read-back of a part happens here), with the seen box."""
    arrays = {k: part[k].cpu().numpy() if torch.is_tensor(part[k]) else np.asarray(part[k]) for k in PART_ARRAYS if part.get(k) is not None}
    if arrays["votes"].dtype != np.uint16 or arrays["votes"].ndim != 3:
        raise ValueError(f"write_mosaic_part: votes must be uint16 [K, CH, CW], got {arrays['votes'].dtype} {arrays['votes'].shape}")
    arrays["origin"], arrays["mask_size"] = np.array(part["origin"], np.int64), np.array(part["mask_size"], np.int64)
    arrays["frames"], arrays["mode"] = np.array(int(part["frames"]), np.int64), np.array(part.get("mode") or "")
    arrays["box"] = np.array(part_seen_box(arrays["poses"], part["mask_size"], arrays["votes"].shape[1:], part["origin"]), np.int64)
    return arrays


def write_mosaic_part(path, part):
    """A mosaic as ONE .npz: mosaic_part()'s arrays, the pose rows, and the seen bounding box taken from the pose rows here on the host."""
    with open(path, "wb") as f:   # a file object: numpy then appends no suffix of its own
        np.savez_compressed(f, **mosaic_part_arrays(part))


def read_mosaic_part(path, device):
    """write_mosaic_part()'s file as the dict FlowPredictor.merge_mosaic() takes, its arrays on `device`."""
    with np.load(path) as z:
        missing = [k for k in ("votes", "state", "poses", "tail", "origin", "mask_size", "frames", "mode", "box") if k not in z.files]
        if missing:
            raise ValueError(f"read_mosaic_part: {path} is no mosaic part: it lacks {missing}")
        part = {k: torch.from_numpy(z[k]).to(device) for k in PART_ARRAYS if k in z.files}
        part.update(rank=part.get("rank"), rgba=part.get("rgba"), origin=tuple(int(v) for v in z["origin"]), mask_size=tuple(int(v) for v in z["mask_size"]),
                    frames=int(z["frames"]), mode=str(z["mode"]) or None, box=tuple(int(v) for v in z["box"]))
    return part


def write_merge_csv(path, names, report):
    """FlowPredictor.merge_report() as a CSV, one row per merged part: its name, the link's status, b_to_a m00 .. m12, the inliers and
    usable rows of the fit that registered it, the status of every register row, and mosaic_merge's counts."""
    links, outs, counts = report
    if len(names) != len(links) or len(outs) != len(links) or len(counts) != len(links):
        raise ValueError(f"write_merge_csv: one name per merged part, got {len(names)} names for {len(links)} links, {len(outs)} out tables and {len(counts)} count rows")
    with open(path, "w", newline="") as f:
        f.write("part,link,m00,m01,m02,m10,m11,m12,inliers,usable,register,reached,voted,votes,taken\n")
        for name, link, out, count in zip(names, np.asarray(links).tolist(), outs, np.asarray(counts).tolist()):
            status = LINK_STATUS[link[12]] if 0 <= link[12] < len(LINK_STATUS) else "out_of_bounds"
            f.write(",".join([str(name), status] + [f"{v / (1 << 20):.6f}" for v in link[:6]] + [str(link[13]), str(link[14]), "/".join(str(int(r[0])) for r in out)]
                             + [str(v) for v in count[1:5]]) + "\n")


# ---- the change between two mosaics of the same ground
# ops.mosaic_change's six codes as ops.ortho_compose draws them (R, G, B, A): "not comparable" and "same" leave the imagery as it is
CHANGE_PALETTE = np.array([[0, 0, 0, 0], [0, 0, 0, 0], [255, 255, 0, 96], [255, 0, 255, 176], [0, 64, 255, 208], [255, 128, 0, 208]], dtype=np.uint8)
_CHANGE_KEYS = {"min_votes", "min_conf", "tolerance", "watch"}
_CHANGE_REGISTER_KEYS = {"rounds", "search", "intra_bias", "fit_rounds", "tol", "min_inliers", "window", "place"}
_CHANGE_REGION_KEYS = {"max_regions", "connectivity", "max_contours", "max_vertices", "simplify_rounds"}


def mosaic_change(part_a, part_b, link=None, register=True, regions=False, min_region_area=0, outlines=False, simplify=None, **options):
    """Where mosaic B differs from mosaic A, in A's canvas (mosaic_part()'s or read_mosaic_part()'s dicts on one device; B is usually the
    later flight).  The two are NOT merged and neither is changed.  register=True: both need an orthophoto, and ops.register_mosaics
    runs on their rgba planes from `link` (default: the identity with status 1; rounds, search, intra_bias, fit_rounds, tol, min_inliers,
    window and place go to it, a place= without b_box taking B's seen box).  register=False: the link is used as given, and only a link
    with status 0 compares anything.  Then ops.mosaic_change with min_votes, min_conf, tolerance and watch.  regions=True: the change
    plane, a mask with the ids 0..5, goes through ops.mask_regions and ops.region_table with classes=6 (min_region_area > 1: and
    ops.region_filter first; outlines=True: ops.region_outlines; simplify=TOL: ops.outline_simplify; max_regions, connectivity,
    max_contours, max_vertices and simplify_rounds as FlowPredictor takes them), so every gained or lost area is a region with area,
    box, centroid and polygon.  -> a dict of device tensors: change, cls_a, cls_b, transitions, counts (ops.mosaic_change's), link, outs
    (register_mosaics' rows, None without), regions = (table, counts, index) or None, outlines and simplified = the ops' tuples or
    None, tolerance = simplify.  Enqueues only; change_report() reads back.  The defaults are guesses, not validated on real video."""
    unknown = set(options) - _CHANGE_KEYS - _CHANGE_REGISTER_KEYS - _CHANGE_REGION_KEYS
    if unknown:
        raise ValueError(f"mosaic_change: unknown options {sorted(unknown)}")
    place = _placed_on_one_mask_size("mosaic_change", part_a, part_b, options.get("place"))
    if part_a["votes"].shape[0] != part_b["votes"].shape[0]:
        raise ValueError(f"mosaic_change: both mosaics must count the same classes, got {part_a['votes'].shape[0]} and {part_b['votes'].shape[0]}")
    if register and (part_a.get("rgba") is None or part_b.get("rgba") is None):
        raise ValueError("mosaic_change: register=True reads both orthophotos (mosaic parts made with ortho=); pass register=False with a registered link otherwise")
    if not register and link is None:
        raise ValueError("mosaic_change: register=False needs the link")
    if (outlines or simplify is not None or min_region_area > 1) and not regions:
        raise ValueError("mosaic_change: min_region_area, outlines and simplify go with regions=True")
    if simplify is not None and not outlines:
        raise ValueError("mosaic_change: simplify= goes with outlines=True")
    dev = part_a["votes"].device
    at, other = tuple(int(v) for v in part_a["origin"]), tuple(int(v) for v in part_b["origin"])
    outs = None
    if register:
        kw = {k: v for k, v in options.items() if k in _CHANGE_REGISTER_KEYS}
        if place is not None:
            kw["place"] = place
        link = ops.mosaic_link(device=dev) if link is None else link.clone()
        link, outs = ops.register_mosaics((part_a["rgba"], at), (part_b["rgba"], other), link, **kw)
    elif set(options) & _CHANGE_REGISTER_KEYS:
        raise ValueError(f"mosaic_change: {sorted(set(options) & _CHANGE_REGISTER_KEYS)} go with register=True")
    change, cls_a, cls_b, transitions, counts = ops.mosaic_change(part_a["votes"], at, part_b["votes"], other, link,
                                                                  **{k: v for k, v in options.items() if k in _CHANGE_KEYS})
    result = dict(change=change, cls_a=cls_a, cls_b=cls_b, transitions=transitions, counts=counts, link=link, outs=outs, regions=None, outlines=None,
                  simplified=None, tolerance=simplify)
    if regions:
        cap, conn = int(options.get("max_regions", 1024)), int(options.get("connectivity", 8))
        mask = change[None]
        labels = ops.mask_regions(mask, ops.CHANGE_CLASSES, conn)
        table, region_counts, index = ops.region_table(mask, labels, ops.CHANGE_CLASSES, None, 128, cap)
        if min_region_area > 1:
            mask = ops.region_filter(mask, index, table, ops.CHANGE_CLASSES, min_region_area)
            labels = ops.mask_regions(mask, ops.CHANGE_CLASSES, conn)
            table, region_counts, index = ops.region_table(mask, labels, ops.CHANGE_CLASSES, None, 128, cap)
            result["change"] = mask[0]
        result["regions"] = (table, region_counts, index)
        if outlines:
            result["outlines"] = ops.region_outlines(index, cap, conn, int(options.get("max_contours", 4096)), int(options.get("max_vertices", 32768)))
            if simplify is not None:
                contours, vertices, _, outline_counts = result["outlines"]
                result["simplified"] = ops.outline_simplify(contours, vertices, outline_counts, simplify, int(options.get("simplify_rounds", 32)))
    return result


def change_report(result):
    """mosaic_change()'s result on the host -- the ONE place that reads back: counts int64 numpy [8], transitions [2, K, K], link [16], outs
    [rows, 8] or None; with regions: rows = [int64 [regions, 10]] as FlowPredictor.region_report() hands a frame's (what
    write_regions_csv and write_outlines_geojson take, with frame_ids = [0]); outlines and simplified as outline_report() and
    simple_outline_report() hand them, for that one frame; shapes = [the regions' (perimeter, contours, vertices)]."""
    host = lambda t: t.cpu().numpy()  # noqa: E731
    report = dict(counts=host(result["counts"]), transitions=host(result["transitions"]), link=host(result["link"]),
                  outs=None if result["outs"] is None else host(result["outs"]), rows=None, outlines=None, simplified=None, shapes=None, tolerance=result["tolerance"])
    if result["regions"] is not None:
        table, counts, _ = result["regions"]
        written = int(host(counts)[0, 1])
        report["rows"] = [host(table)[0, :written]]
        if result["outlines"] is not None:
            contours, vertices, shape, c = (host(t) for t in result["outlines"])
            total = 0 if c[0, 3] & 1 else int(c[0, 2])
            report["outlines"] = ([(contours[0, :int(c[0, 1])], vertices[0, :total], shape[0, :written])], c[:, 3])
            report["shapes"] = [shape[0, :written]]
            if result["simplified"] is not None:
                simple, kept, sc = (host(t) for t in result["simplified"])
                report["simplified"] = ([(simple[0, :int(sc[0, 0])], kept[0, :int(sc[0, 1])])], sc)
    return report


def write_change_csv(path, report, class_names=None):
    """change_report()'s counts and transitions as one CSV of two tables.  First one row per class pair that has a comparable pixel: the
    class in A (`from`), the class in B (`to`), the comparable pixels and of those the changed ones (code >= 3: not the same and not
    explained by the tolerance).  Then, after an empty line, the eight counts by name."""
    counts, pairs = np.asarray(report["counts"]).tolist(), np.asarray(report["transitions"])
    k = pairs.shape[1]
    name = (lambda c: str(c)) if class_names is None else (lambda c: str(class_names[c]))
    with open(path, "w", newline="") as f:
        f.write("from,to,comparable,changed\n")
        for ca in range(k):
            for cb in range(k):
                if pairs[0, ca, cb]:
                    f.write(f"{name(ca)},{name(cb)},{int(pairs[0, ca, cb])},{int(pairs[1, ca, cb])}\n")
        f.write("\nlink,reached,comparable," + ",".join(ops.CHANGE_CODES[1:]) + "\n")
        f.write(",".join([LINK_STATUS[counts[0]] if 0 <= counts[0] < len(LINK_STATUS) else "out_of_bounds"] + [str(v) for v in counts[1:]]) + "\n")


def change_image(result, rgba=None, palette=CHANGE_PALETTE, fill=(0, 0, 0)):
    """The change plane drawn over mosaic A's orthophoto (rgba = part_a["rgba"]) through ops.ortho_compose, or over a plain fill without
    one -> uint8 [CH, CW, 3] on the device.  Codes 0 and 1 of CHANGE_PALETTE have alpha 0: only what differs is drawn."""
    change = result["change"]
    if rgba is None:
        rgba = torch.zeros(tuple(change.shape), dtype=torch.int32, device=change.device)  # never seen: the fill shows everywhere
    return ops.ortho_compose(rgba, change, palette, fill=fill)


def write_change_png(path, result, rgba=None, palette=CHANGE_PALETTE, fill=(0, 0, 0)):
    """change_image() as a PNG (the read-back of the picture happens here)."""
    from PIL import Image

    Image.fromarray(change_image(result, rgba, palette, fill).cpu().numpy()).save(path)


# ---- dry-route reachability on the mosaic
ACCESS_COST = {4: 1, 0: 2, 2: 6, 3: 2}   # Street 1, Background 2, Tree 6, Building 2 (the step onto its wall); Water and unseen ground 0: barriers.  A guess
ACCESS_TERMINAL = (3,)            # Building: arrived at, never crossed
ACCESS_MAX_ROUNDS = 4096          # the round limit of mosaic_access by default.  A guess: a route that crosses more tiles than this stays unconverged
ACCESS_MOVES = ((-1, 0, 5), (1, 0, 5), (0, -1, 5), (0, 1, 5), (-1, -1, 7), (1, -1, 7), (-1, 1, 7), (1, 1, 7))   # csrc/access_defs.h's move table: (dx, dy, step)
ACCESS_CUT_OFF = (255, 0, 255)    # write_access_png: a terminal region that no route reaches
_ACCESS_KEYS = {"connectivity", "max_cost", "max_regions", "chunk", "max_rounds", "want_origin"}


def access_seeds(cls, seeds):
    """The seed plane of mosaic_access, uint8 like cls [CH, CW], on cls' device.  seeds: "border" (the seen pixels with an unseen or no
    4-neighbour: where ground the flight never saw begins), or a dict with any of points = [(x, y), ...] canvas pixels, classes = class
    ids, border = True."""
    spec = dict(border=True) if isinstance(seeds, str) and seeds == "border" else seeds
    if not isinstance(spec, dict) or not spec or set(spec) - {"points", "classes", "border"}:
        raise ValueError(f"mosaic_access: seeds must be \"border\" or a dict with points, classes and/or border, got {seeds!r}")
    ch, cw = cls.shape
    plane = torch.zeros((ch, cw), dtype=torch.uint8, device=cls.device)
    points = [tuple(int(v) for v in p) for p in spec.get("points", ())]
    if any(len(p) != 2 or not (0 <= p[0] < cw and 0 <= p[1] < ch) for p in points):
        raise ValueError(f"mosaic_access: seed points must be (x, y) inside the {ch} x {cw} canvas, got {list(spec['points'])}")
    if points:
        at = torch.tensor(points, dtype=torch.int64, device=cls.device)
        plane[at[:, 1], at[:, 0]] = 1
    ids = [int(c) for c in spec.get("classes", ())]
    if any(not 0 <= c <= 31 for c in ids):
        raise ValueError(f"mosaic_access: seed classes must be class ids 0..31, got {ids}")
    for c in ids:
        plane |= (cls == c).to(torch.uint8)
    if spec.get("border"):
        seen = torch.nn.functional.pad(cls != 255, (1, 1, 1, 1), value=False)
        inner = seen[1:-1, 2:] & seen[1:-1, :-2] & seen[2:, 1:-1] & seen[:-2, 1:-1]
        plane |= (seen[1:-1, 1:-1] & ~inner).to(torch.uint8)
    return plane


def mosaic_access(part_or_builder, seeds="border", cost=None, terminal=ACCESS_TERMINAL, min_votes=1, regions=True, **options):
    """Which ground of a mosaic can be reached over ground that is not under water, and at what cost.  part_or_builder: a
    MosaicBuilder or a part (part()'s or read_mosaic_part()'s dict).  The class plane is ops.mosaic_resolve's winner where the pixel has
    min_votes votes, 255 otherwise: unseen ground is a barrier.  seeds: see access_seeds.  cost: {class id: 0..255}, by default Street 1,
    Background 2, Tree 6, Building 2, Water 0 = barrier; terminal: classes that are arrived at but never crossed, by default Building.
    ops.mask_access then runs in chunks of `chunk` rounds (default ops.ACCESS_ROUNDS), the 16 bytes of its status read back after each,
    until it says converged or max_rounds (default 4096) rounds are enqueued; connectivity, max_cost and want_origin go to it.
    regions=True: the class plane goes through ops.mask_regions and ops.region_table (max_regions, default 1024) and ops.region_access
    tabulates the field per region.  -> a dict: cls, seeds, d, origin, status (device tensors), converged (bool: False means every
    value is only an upper bound), rounds (enqueued), regions = (table, counts, index) or None, reach and rows (ops.region_access') or
    None, cost (the 32 costs), terminal, connectivity, classes.
    Costs are mask pixels of the anchor frame in tenths on the 5-7 chamfer metric, not metres.  The default costs and the round limit are
    guesses, not validated on real video."""
    unknown = set(options) - _ACCESS_KEYS
    if unknown:
        raise ValueError(f"mosaic_access: unknown options {sorted(unknown)}")
    part = part_or_builder.part() if hasattr(part_or_builder, "part") else part_or_builder
    votes = part["votes"]
    if not 1 <= int(min_votes) <= 65535:
        raise ValueError(f"mosaic_access: min_votes must be 1..65535, got {min_votes}")
    table = ops.access_cost_table(ACCESS_COST if cost is None else cost, "mosaic_access")
    terminal = tuple(int(c) for c in terminal)
    ops.class_set(terminal, "terminal", "mosaic_access", allow_empty=True)
    conn, chunk, limit = int(options.get("connectivity", 8)), int(options.get("chunk", ops.ACCESS_ROUNDS)), int(options.get("max_rounds", ACCESS_MAX_ROUNDS))
    if conn not in (4, 8):
        raise ValueError(f"mosaic_access: connectivity must be 4 or 8, got {conn}")
    if not 1 <= chunk <= 65535 or limit < 1:
        raise ValueError(f"mosaic_access: chunk must be 1..65535 rounds and max_rounds at least 1, got {chunk} and {limit}")
    cls, _, seen, _ = ops.mosaic_resolve(votes)
    if int(min_votes) > 1:
        cls = torch.where(seen >= int(min_votes), cls, torch.full_like(cls, 255))
    plane = access_seeds(cls, seeds)
    kw = dict(terminal=terminal, connectivity=conn, max_cost=int(options.get("max_cost", 0)), want_origin=bool(options.get("want_origin", True)))
    mask, planes, rounds, converged = cls[None], None, 0, False
    while not converged and rounds < limit:
        step = min(chunk, limit - rounds)
        d, origin, status = ops.mask_access(mask, plane[None], table, rounds=step, resume=planes, **kw)
        planes, rounds = (d, origin), rounds + step
        converged = bool(status[0, 0].item())  # the read-back of 16 bytes per chunk: only here, at report time
    result = dict(cls=cls, seeds=plane, d=d[0], origin=None if origin is None else origin[0], status=status[0], converged=converged, rounds=rounds, regions=None,
                  reach=None, rows=None, cost=table, terminal=terminal, connectivity=conn, classes=int(votes.shape[0]))
    if regions:
        k, cap = int(votes.shape[0]), int(options.get("max_regions", 1024))
        labels = ops.mask_regions(mask, k, conn)
        region_table, region_counts, index = ops.region_table(mask, labels, k, None, 128, cap)
        result["regions"] = (region_table, region_counts, index)
        result["reach"], result["rows"] = ops.region_access(mask, d, origin, index, region_counts, k, cap)
    return result


def access_report(result):
    """mosaic_access()'s result on the host: cls uint8 [CH, CW], d uint32 (ops.ACCESS_NONE: no value), origin int32 or None, status [4],
    converged, rounds, table = region_table's rows [regions, 10], rows = region_access' [regions, 8], reach [K, 4], index int32 [CH, CW] = the
    row of every pixel's region (all None without regions),
    and cost, terminal, connectivity, classes as mosaic_access holds them."""
    host = lambda t: t.cpu().numpy()  # noqa: E731
    report = {k: result[k] for k in ("converged", "rounds", "cost", "terminal", "connectivity", "classes")}
    report.update(cls=host(result["cls"]), d=host(result["d"]).view(np.uint32), origin=None if result["origin"] is None else host(result["origin"]),
                  status=host(result["status"]), table=None, rows=None, reach=None, index=None)
    if result["regions"] is not None:
        table, counts, index = result["regions"]
        written = int(host(counts)[0, 1])
        report.update(table=host(table)[0, :written], rows=host(result["rows"])[0, :written], reach=host(result["reach"])[0], index=host(index)[0])
    return report


def write_access_csv(path, report, class_names=None):
    """access_report()'s regions as a CSV, one row per region: its row number, class, area and centroid (region_table's), its state --
    reached or cut_off; from a field that did not converge reached_bound (the cost is an upper bound) or not_reached_yet -- and for a
    reached one the cost of the cheapest route to it, the pixel of the region that route arrives at, the seed it starts from and that
    seed's region row (empty: none).  Costs are tenths of a mask pixel of the anchor frame on the 5-7 chamfer metric, times the classes'
    costs: not metres."""
    if report["table"] is None:
        raise ValueError("write_access_csv: the result has no regions (mosaic_access(regions=True))")
    name = (lambda c: str(c)) if class_names is None else (lambda c: str(class_names[c]))
    done = bool(report["converged"])
    with open(path, "w", newline="") as f:
        f.write("region,class,area,centroid_x,centroid_y,state,cost,at_x,at_y,origin_x,origin_y,origin_region\n")
        for r, (t, a) in enumerate(zip(np.asarray(report["table"]).tolist(), np.asarray(report["rows"]).tolist())):
            reached = a[0] >= 0
            state = ("reached" if done else "reached_bound") if reached else ("cut_off" if done else "not_reached_yet")
            route = [str(v) if reached else "" for v in a[:5]] + [str(a[5]) if reached and a[5] >= 0 else ""]
            f.write(",".join([str(r), name(t[0]), str(t[1]), f"{t[6] / t[1]:.2f}", f"{t[7] / t[1]:.2f}", state] + route) + "\n")


def access_image(report, palette=ops.FLOOD_PALETTE, fill=(0, 0, 0), cut_off=ACCESS_CUT_OFF):
    """The cost field as a ramp over the class colours, drawn on the host -> uint8 numpy [CH, CW, 3].  A pixel with a value keeps between
    all (cost 0) and a third (the largest cost) of its class colour's brightness; a pixel without one is drawn at a sixth of it; unseen
    ground is `fill`; the regions of the terminal classes that no route reaches (with regions=True) are `cut_off`."""
    cls, d = report["cls"], report["d"]
    colours = np.array([fill] * 256, np.float64)
    colours[:len(palette)] = np.array(palette, np.float64)
    base = colours[cls]
    has = d != ops.ACCESS_NONE
    top = max(int(d[has].max()) if has.any() else 0, 1)
    t = np.where(has, d.astype(np.float64) / top, 0.0)[..., None]
    img = np.where(has[..., None], base * (1.0 - t * 2 / 3), base / 6.0)
    img[cls == 255] = fill
    if report["table"] is not None:
        lost = [r for r, (t, a) in enumerate(zip(report["table"].tolist(), report["rows"].tolist())) if t[0] in report["terminal"] and a[0] < 0]
        img[np.isin(report["index"], lost)] = cut_off
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def write_access_png(path, report, **kw):
    """access_image() as a PNG."""
    from PIL import Image

    Image.fromarray(access_image(report, **kw)).save(path)


def access_route(report, x, y):
    """The route from a seed to canvas pixel (x, y), read backwards off the field on the host: from (x, y), at every pixel p the first
    neighbour q, in the move table's order, with an allowed move q -> p and d[q] + move == d[p], until a pixel with d = 0.  O(route
    length).  -> [(x, y), ..., (seed_x, seed_y)].  Needs a converged field; a pixel without a value has no route."""
    cls, d, cost, conn = report["cls"], report["d"], report["cost"], report["connectivity"]
    if not report["converged"]:
        raise ValueError("access_route: the field has not converged: its values are upper bounds, not route costs")
    ch, cw = cls.shape
    x, y = int(x), int(y)
    if not (0 <= x < cw and 0 <= y < ch) or d[y, x] == ops.ACCESS_NONE:
        raise ValueError(f"access_route: ({x}, {y}) has no value")
    terminal = set(int(k) for k in report["terminal"])
    walk = lambda px, py: 0 <= px < cw and 0 <= py < ch and cls[py, px] < 32 and cost[cls[py, px]] > 0 and int(cls[py, px]) not in terminal  # noqa: E731
    chain = [(x, y)]
    while d[y, x] != 0:
        for dx, dy, step in ACCESS_MOVES[:8 if conn == 8 else 4]:
            qx, qy = x + dx, y + dy
            if not walk(qx, qy) or d[qy, qx] == ops.ACCESS_NONE or (dx and dy and not (walk(qx, y) and walk(x, qy))):
                continue
            if int(d[qy, qx]) + step * (cost[cls[qy, qx]] + cost[cls[y, x]]) == int(d[y, x]):
                x, y = qx, qy
                break
        else:
            raise ValueError(f"access_route: no neighbour of ({x}, {y}) explains its value")
        chain.append((x, y))
    return chain


def write_access_geojson(path, report):
    """One LineString per reached region of a terminal class: access_route() from the region's cheapest pixel to its seed, in canvas
    pixel centres (x + 0.5, y + 0.5), with the region's row, class and cost as properties."""
    import json

    if report["table"] is None:
        raise ValueError("write_access_geojson: the result has no regions (mosaic_access(regions=True))")
    features = []
    for r, (t, a) in enumerate(zip(np.asarray(report["table"]).tolist(), np.asarray(report["rows"]).tolist())):
        if t[0] in report["terminal"] and a[0] >= 0:
            chain = access_route(report, a[1], a[2])
            features.append(dict(type="Feature", properties=dict(region=r, cls=t[0], cost=a[0]),
                                 geometry=dict(type="LineString", coordinates=[[px + 0.5, py + 0.5] for px, py in chain])))
    with open(path, "w") as f:
        json.dump(dict(type="FeatureCollection", features=features), f)


# ---- the mosaic in metres
_GROUND_KEYS = {"max_regions", "connectivity", "max_contours", "max_vertices", "simplify_rounds", "fill", "rgb_fill", "raster"}


def mosaic_ground(part_or_builder, model, gsd=None, regions=False, outlines=False, simplify=None, min_votes=1, change=None, **options):
    """The mosaic in map coordinates.  part_or_builder: a MosaicBuilder or a part (part()'s or read_mosaic_part()'s dict);
    model: a flow.georef.GroundModel fitted in THIS canvas (GroundModel.fit(..., origin=part["origin"])).  The id plane is
    ops.mosaic_resolve's class plane (255 where a pixel has fewer than min_votes votes), or, with change = mosaic_change()'s result in this
    part's canvas, its change plane with the six ids of ops.CHANGE_CODES: gained and lost water in m^2.  Then ops.ground_area; with
    regions=True ops.mask_regions and ops.region_table on the plane (max_regions, connectivity) and the areas per region; with
    outlines=True ops.region_outlines (max_contours, max_vertices), simplify=TOL ops.outline_simplify (simplify_rounds), and
    ops.ground_points on the vertices; and ops.ground_rectify of the plane, the confidence plane and, where the part has one, the
    orthophoto, onto the north-up raster model.raster() gives for gsd metres (default: the model's mean pixel size, rounded to
    millimetres; raster=False: no raster).  fill and rgb_fill go to ops.ground_rectify.  -> a dict of device tensors and plain numbers;
    enqueues only, ground_report() reads back.  A planar model over an affine pose chain: the chain's drift and parallax are in the
    result; no DEM, no lens model; not validated on real video or against surveyed points."""
    unknown = set(options) - _GROUND_KEYS
    if unknown:
        raise ValueError(f"mosaic_ground: unknown options {sorted(unknown)}")
    if not (hasattr(model, "forward") and hasattr(model, "inverse") and hasattr(model, "raster")):
        raise ValueError(f"mosaic_ground: model must be a flow.georef.GroundModel, got {model!r}")
    part = part_or_builder.part() if hasattr(part_or_builder, "part") else part_or_builder
    if not 1 <= int(min_votes) <= 65535:
        raise ValueError(f"mosaic_ground: min_votes must be 1..65535, got {min_votes}")
    if (outlines or simplify is not None) and not regions:
        raise ValueError("mosaic_ground: outlines and simplify go with regions=True")
    if simplify is not None and not outlines:
        raise ValueError("mosaic_ground: simplify= goes with outlines=True")
    if gsd is not None and not (float(gsd) * 1000.0 >= 1.0 and round(float(gsd) * 1000.0) <= ops.GROUND_MAX_GSD_MM):
        raise ValueError(f"mosaic_ground: gsd must be 0.001 .. {ops.GROUND_MAX_GSD_MM / 1000.0} metres, got {gsd}")
    votes, origin = part["votes"], tuple(int(v) for v in part["origin"])
    size = tuple(int(v) for v in votes.shape[1:])
    cls, conf, seen, _ = ops.mosaic_resolve(votes)
    if int(min_votes) > 1:
        cls = torch.where(seen >= int(min_votes), cls, torch.full_like(cls, 255))
    plane, k = cls, int(votes.shape[0])
    if change is not None:
        plane, k = change["change"], ops.CHANGE_CLASSES
        if tuple(plane.shape) != size:
            raise ValueError(f"mosaic_ground: the change plane {tuple(plane.shape)} is not of this mosaic's canvas {size} (mosaic A's is the one it is made in)")
    result = dict(model=model, origin=origin, size=size, classes=k, plane=plane, conf=conf, changed=change is not None, regions=None, outlines=None,
                  simplified=None, tolerance=simplify, points=None, simple_points=None, raster=None)
    index, cap = None, 0
    if regions:
        cap, conn = int(options.get("max_regions", 1024)), int(options.get("connectivity", 8))
        labels = ops.mask_regions(plane[None], k, conn)
        table, region_counts, index = ops.region_table(plane[None], labels, k, None, 128, cap)
        result["regions"] = (table, region_counts, index)
        if outlines:
            result["outlines"] = ops.region_outlines(index, cap, conn, int(options.get("max_contours", 4096)), int(options.get("max_vertices", 32768)))
            contours, vertices, _, outline_counts = result["outlines"]
            result["points"] = ops.ground_points(vertices[0], model, origin)
            if simplify is not None:
                result["simplified"] = ops.outline_simplify(contours, vertices, outline_counts, simplify, int(options.get("simplify_rounds", 32)))
                result["simple_points"] = ops.ground_points(result["simplified"][1][0], model, origin)
    result["class_area2"], result["region_area2"], result["counts"] = ops.ground_area(plane, model, origin, k, None if index is None else index[0], cap)
    if options.get("raster", True):
        raster_size, gsd_mm, top_left = model.raster(size, origin, None if gsd is None else int(round(float(gsd) * 1000.0)))
        planes, rgb = ops.ground_rectify(model, origin, raster_size, gsd_mm, top_left, (plane, conf), part.get("rgba"), int(options.get("fill", 255)),
                                         tuple(options.get("rgb_fill", (0, 0, 0))))
        result["raster"] = dict(size=raster_size, gsd_mm=gsd_mm, top_left_mm=top_left, plane=planes[0], conf=planes[1], rgb=rgb)
    return result


def ground_report(result):
    """mosaic_ground()'s result on the host -- the ONE place that reads back.  -> a dict: classes = one row per id (id, pixels' area in
    m^2, share of the summed area); summed_m2; counts = ops.ground_area's (pixels summed, folded, ids beyond the classes, 0); regions =
    one row per region (row, id, pixels, m^2, centroid E, centroid N) or None -- the centroid is region_table's pixel centroid taken
    through the model; rings = {region row: [ring, ...]} of (E, N) metres, the outer ring first, each closed, simplified ones where
    simplify was given (None without outlines; `flags` = region_outlines' for the frame); raster = dict(plane, conf, rgb (numpy),
    gsd_mm, top_left_mm, world = the world file's six numbers) or None; model, rms, residuals (the fit's, metres), crs."""
    host = lambda t: t.cpu().numpy()  # noqa: E731
    model = result["model"]
    class_area2, counts = host(result["class_area2"]), host(result["counts"])
    total = int(class_area2.sum())
    report = dict(model=model, rms=model.rms, residuals=model.residuals, crs=model.crs, counts=counts, changed=result["changed"],
                  classes=[(k, a / 2e6, (a / total if total else 0.0)) for k, a in enumerate(class_area2.tolist())], summed_m2=total / 2e6, regions=None,
                  rings=None, flags=0, tolerance=result["tolerance"], raster=None)
    if result["regions"] is not None:
        table, region_counts, _ = result["regions"]
        written = int(host(region_counts)[0, 1])
        rows, area2 = host(table)[0, :written], host(result["region_area2"])[:written]
        centre = np.array([[t[6] / t[1] + 0.5, t[7] / t[1] + 0.5] for t in rows.tolist()], np.float64).reshape(-1, 2)   # continuous canvas coordinates
        en =model.to_ground(centre, result["origin"])
        report["regions"] = [(r, int(t[0]), int(t[1]), int(a) / 2e6, float(c[0]), float(c[1])) for r, (t, a, c) in enumerate(zip(rows.tolist(), area2.tolist(), en))]
        if result["outlines"] is not None:
            contours, _, _, c = (host(t) for t in result["outlines"])
            report["flags"] = int(c[0, 3])
            rings = {}
            if not int(c[0, 3]) & 1:
                rows6 = contours[0, :int(c[0, 1])].tolist()
                if result["simplified"] is not None:
                    simple, _, sc = (host(t) for t in result["simplified"])
                    spans = [(s[0], s[1]) for s in simple[0, :int(sc[0, 0])].tolist()]
                    mm = host(result["simple_points"])
                else:
                    spans = [(row[1], row[2]) for row in rows6]
                    mm = host(result["points"])
                for row, (first, count) in zip(rows6, spans):
                    ring = model.mm_to_en(mm[first:first + count]).tolist()
                    if not ring:
                        continue
                    ring.append(ring[0])
                    if row[4] > 0:
                        rings.setdefault(row[0], []).insert(0, ring)
                    else:
                        rings.setdefault(row[0], []).append(ring)
            report["rings"] = rings
    if result["raster"] is not None:
        r = result["raster"]
        report["raster"] = dict(plane=host(r["plane"]), conf=host(r["conf"]), rgb=None if r["rgb"] is None else host(r["rgb"]), gsd_mm=r["gsd_mm"],
                                top_left_mm=r["top_left_mm"], world=model.world_file(r["gsd_mm"], r["top_left_mm"]))
    return report


def write_ground_csv(path, report, class_names=None):
    """ground_report() as one CSV of up to three tables: one row per id (its name, m^2, hectares, share of the summed area); after an
    empty line the fit (kind, control points, RMS and largest residual in metres, CRS, folded pixels); and, with regions, one row per
    region (row, id, pixels, m^2, centroid easting and northing in metres)."""
    codes = ops.CHANGE_CODES if report["changed"] else class_names
    name = (lambda c: str(c)) if codes is None else (lambda c: str(codes[c]) if c < len(codes) else str(c))
    model = report["model"]
    worst = float(np.sqrt((model.residuals ** 2).sum(axis=1)).max()) if len(model.residuals) else 0.0
    with open(path, "w", newline="") as f:
        f.write("class,area_m2,hectares,share\n")
        for k, m2, share in report["classes"]:
            f.write(f"{name(k)},{m2:.6f},{m2 / 1e4:.6f},{share:.6f}\n")
        f.write("\nkind,points,rms_m,max_residual_m,crs,folded_pixels\n")
        f.write(f"{model.kind},{len(model.residuals)},{model.rms:.6f},{worst:.6f},{model.crs or ''},{int(report['counts'][1])}\n")
        if report["regions"] is not None:
            f.write("\nregion,class,pixels,area_m2,centroid_e,centroid_n\n")
            for r, k, pixels, m2, e, n in report["regions"]:
                f.write(f"{r},{name(k)},{pixels},{m2:.6f},{e:.3f},{n:.3f}\n")


def ground_image(report, what="class", palette=ops.FLOOD_PALETTE, fill=(0, 0, 0)):
    """The rectified raster as a picture, uint8 numpy [GH, GW, 3]: what = "class" (the id plane through the palette; CHANGE_PALETTE's
    colours for a change plane), "ortho" (the rectified orthophoto) or "conf" (the confidence plane as grey)."""
    r = report["raster"]
    if r is None:
        raise ValueError("ground_image: the result has no raster (mosaic_ground(raster=True))")
    if what == "ortho":
        if r["rgb"] is None:
            raise ValueError("ground_image: the mosaic has no orthophoto (a builder made with ortho=)")
        return r["rgb"]
    if what == "conf":
        return np.repeat(r["conf"][..., None], 3, axis=2)
    if what != "class":
        raise ValueError(f"ground_image: what must be class, ortho or conf, got {what!r}")
    colours = np.array([fill] * 256, np.uint8)
    table = CHANGE_PALETTE[:, :3] if report["changed"] else np.array(palette, np.uint8)
    colours[:len(table)] = table
    return colours[r["plane"]]


def write_ground_png(path, report, what="class", **kw):
    """ground_image() as a PNG with its world file beside it (the PNG's name with the extension .pgw): six lines -- gsd, 0, 0, -gsd, and
    the easting and northing of the top-left pixel's CENTRE -- in metres."""
    from PIL import Image

    Image.fromarray(ground_image(report, what, **kw)).save(path)
    stem = path[:-4] if path.lower().endswith(".png") else path
    with open(stem + ".pgw", "w") as f:
        f.write("".join(f"{v!r}\n" for v in report["raster"]["world"]))


def write_ground_geojson(path, report, class_names=None):
    """The regions as one GeoJSON FeatureCollection in map coordinates: one Polygon per region with an outer ring, the outer ring first,
    then its holes, in eastings and northings (metres); properties region, class, pixels, area_m2; the model's CRS name in a `crs`
    member (the pre-2016 GeoJSON form, which GIS software still reads), left out without a name."""
    import json

    if report["rings"] is None:
        raise ValueError("write_ground_geojson: the result has no outlines (mosaic_ground(regions=True, outlines=True))")
    codes = ops.CHANGE_CODES if report["changed"] else class_names
    features = []
    for r, k, pixels, m2, e, n in report["regions"]:
        if r in report["rings"]:
            props = {"region": r, "class": k if codes is None or k >= len(codes) else str(codes[k]), "pixels": pixels, "area_m2": m2, "centroid": [e, n]}
            features.append(dict(type="Feature", properties=props, geometry=dict(type="Polygon", coordinates=report["rings"][r])))
    doc = dict(type="FeatureCollection", features=features)
    if report["crs"]:
        doc["crs"] = dict(type="name", properties=dict(name=report["crs"]))
    if report["tolerance"] is not None:
        doc["tolerance"] = report["tolerance"]
    with open(path, "w") as f:
        json.dump(doc, f)


def write_mosaic_csv(path, frame_ids, poses, totals, refine=None):
    """FlowPredictor.mosaic_report()'s poses int64 [frames, 16] and totals int64 [K, 2] as one CSV of two tables.  First one row per
    frame: frame id, status (ok, bridged, lost), clipped (1: a corner of the frame lies outside the canvas), inliers and usable rows of
    the pair's fit, and the pose m00 .. m12 that takes a mask pixel of the frame to the anchor frame's pixels (empty for a lost frame).
    Then, after an empty line, one row per class: the canvas pixels it won, their share of the seen pixels, and its votes.  Pixels are
    mask pixels of the anchor frame, not metres.  refine: FlowPredictor.refine_report()'s int64 [frames, 8]; the frame rows then end with
    refine (corrected, skipped, no_fit, out_of_bounds, lost), the usable rows and inliers of the fit against the map, and its shift in
    mask pixels."""
    poses, totals = np.asarray(poses), np.asarray(totals)
    if refine is not None and np.asarray(refine).shape != (poses.shape[0], 8):
        raise ValueError(f"write_mosaic_csv: refine must be [frames, 8] with one row per pose row, got {np.asarray(refine).shape} for {poses.shape[0]} frames")
    extra = [[]] * poses.shape[0] if refine is None else [
        [REFINE_STATUS[r[0]] if 0 <= r[0] <= 4 else "lost", str(r[1]), str(r[2]), f"{r[4] / (1 << 20):.6f}", f"{r[5] / (1 << 20):.6f}"] for r in np.asarray(refine).tolist()]
    if poses.ndim != 2 or poses.shape[1] != 16 or len(frame_ids) != poses.shape[0] or totals.ndim != 2 or totals.shape[1] != 2:
        raise ValueError(f"write_mosaic_csv: poses must be [frames, 16] with one frame id per row and totals [K, 2], got {poses.shape}, {len(frame_ids)} "
                         f"ids and {totals.shape}")
    seen = int(totals[:, 0].sum())
    with open(path, "w", newline="") as f:
        f.write("frame,status,clipped,inliers,usable,m00,m01,m02,m10,m11,m12" + (",refine,refine_usable,refine_inliers,refine_dx,refine_dy" if refine is not None else "")
                + "\n")
        for fid, row, more in zip(frame_ids, poses.tolist(), extra):
            status = row[12] if 0 <= row[12] <= 2 else 2
            pose = [f"{v / (1 << 20):.6f}" for v in row[:6]] if status != 2 else [""] * 6
            f.write(",".join([str(int(fid)), MOSAIC_STATUS[status], str(row[13]), str(row[14]), str(row[15])] + pose + more) + "\n")
        f.write("\nclass,pixels,share,votes\n")
        for k, (pixels, votes) in enumerate(totals.tolist()):
            f.write(f"{k},{pixels},{pixels / seen if seen else 0.0:.6f},{votes}\n")
