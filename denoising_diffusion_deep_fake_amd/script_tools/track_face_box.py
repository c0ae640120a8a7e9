"""Write the face-box track of a video from boxes marked by hand at key frames: the file that
put_video_through_fake_model --track and video_to_center_cropped_images --track read.  There is no detector: the box of a
key frame is the template, and the device follows it from frame to frame (ops.track_template_u8: a reduced grey image of
every frame, then the smallest sum of absolute differences in a search window).  The box keeps the key's size unless
--scale is given: then the size is searched too, one sample of the template's longer side a frame (about 2 %), and the
box follows a face that walks towards the camera or away from it (ops.track_template_scale_u8).  What remains: the
template's longer side stays within 4..64 samples at the key's stride (a third over the default side of 48).  Where
the face outgrows that, where the tracker drifts and behind a cut, mark another key frame -- the tracker is seeded anew
at every key.  Head roll: --rotate searches the box's angle too, one step (--rotate-step, 2 degrees) a frame, up to
--rotate-max degrees either way (ops.track_template_rot_u8), and writes it as a fifth column, which the two tools read with
--track-rotate; the angle is relative to the key frame's pose unless --key-angle K A gives the roll at that key.  Without
--rotate the roll is marked by hand: --key-angle K A (repeatable) writes the fifth column from the key angles, interpolated
linearly.  --rotate and --scale cannot be combined: the rotation search keeps the key's size.
A face that leaves the search window -- out of the frame and back on the other side, a cut away and back, a hand in front
of it -- is lost for good without --reacquire [RELOST]: with it, a frame that the window does not find is looked for in the
whole frame with the key box's own template, and taken from there when that costs at most RELOST (default 8) grey levels
a sample (ops.track_template_reacq_u8); the frame is written as an ordinary `x y w h` line, and one line on stderr counts
the found, re-acquired and lost frames.  --reacquire cannot be combined with --scale or --rotate.

    python -m d3f.script_tools.track_face_box VIDEO --key K X Y W H [--key ...] [-o FILE]
                                              [--scale | --rotate | --reacquire [RELOST]] [--key-angle K A ...]
"""
import argparse
import sys
from pathlib import Path

import torch

from .. import _lib, ops
from .video_writer_context_manager import batches, import_cv2, open_video_as_generator


def main():

    args = parse_command_line_arguments()

    tracker = TrackFaceBox(
        args.video_path,
        args.key,
        output_path=args.output,
        batch_frames=args.batch_frames,
        search=args.search,
        adapt=args.adapt,
        lost=args.lost,
        template_side=args.template_side,
        scale=args.scale,
        scale_penalty=args.scale_penalty,
        key_angles=args.key_angle,
        rotate=args.rotate,
        rotate_step=args.rotate_step,
        rotate_max=args.rotate_max,
        rotate_penalty=args.rotate_penalty,
        reacquire=args.reacquire,
        )
    found = sum(box is not None for box in tracker.track)
    print(f"{tracker.output_path}: {len(tracker.track)} frames, the face found in {found}")
    if args.reacquire is not None:
        print(tracker.summary(), file=sys.stderr)


def parse_command_line_arguments(argv=None):
    parser = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)

    parser.add_argument("video_path", help="path to the video")
    parser.add_argument("--key", type=int, nargs=5, action="append", metavar=("K", "X", "Y", "W", "H"), required=True,
                        help="the face box x y w h, in pixels, marked at frame K (counted from 0); repeat it to correct "
                             "drift, a cut or a change of size: the tracker starts anew at every key")
    parser.add_argument("-o", "--output", default=None, metavar="FILE",
                        help="the track file (default: <video stem>_track.txt next to the video)")
    parser.add_argument("--batch-frames", type=int, default=8, help="frames per device call (the file does not depend on it)")
    parser.add_argument("--search", type=int, default=ops.TRACK_SEARCH, metavar="R",
                        help=f"search radius per frame in pixels of the reduced image, 1..{_lib.TRACK_MAX_SEARCH} "
                             f"(default {ops.TRACK_SEARCH})")
    parser.add_argument("--adapt", type=int, default=ops.TRACK_ADAPT, metavar="A",
                        help=f"eighths of the found window blended into the template per frame, 0..8 (default {ops.TRACK_ADAPT})")
    parser.add_argument("--lost", type=int, default=ops.TRACK_LOST, metavar="L",
                        help=f"mean absolute difference in grey levels above which a frame is written as `-`, 0..255 "
                             f"(default {ops.TRACK_LOST})")
    parser.add_argument("--template-side", type=int, default=ops.TRACK_TEMPLATE_SIDE, metavar="S",
                        help=f"the template's longer side in samples, 4..{_lib.TRACK_MAX_SIDE} (default "
                             f"{ops.TRACK_TEMPLATE_SIDE})")

    parser.add_argument("--scale", action="store_true",
                        help="search the size of the box too, one level (one sample of the template's longer side) a frame; "
                             "without it the box keeps the key's size")
    parser.add_argument("--scale-penalty", type=int, default=ops.TRACK_SCALE_PENALTY, metavar="P",
                        help=f"with --scale: what a change of size must win by, in 1/4096 grey levels per sample, "
                             f"0..{_lib.TRACK_MAX_SCALE_PENALTY} (default {ops.TRACK_SCALE_PENALTY})")

    parser.add_argument("--key-angle", nargs=2, action="append", metavar=("K", "A"), default=None,
                        help="the head's roll at frame K, A in decimal degrees (positive: clockwise on the screen); repeat "
                             "it.  The file gains a fifth column, the linear interpolation of the key angles (constant "
                             "before the first and after the last), for --track-rotate.  With --rotate: the roll at the key "
                             "frame K, which must have a --key; the tracker follows it from there")
    parser.add_argument("--rotate", action="store_true",
                        help="search the angle of the box too, one step a frame, and write it as the fifth column; without "
                             "it the tracker does not search rotation")
    parser.add_argument("--rotate-step", type=int, default=ops.TRACK_ROT_STEP, metavar="H",
                        help=f"with --rotate: the angle of one step in hundredths of a degree (default {ops.TRACK_ROT_STEP})")
    parser.add_argument("--rotate-max", type=int, default=ops.TRACK_ROT_MAX, metavar="D",
                        help=f"with --rotate: the angle stays within +-D degrees, at most {_lib.TRACK_ROT_MAX_INDEX} steps "
                             f"(default {ops.TRACK_ROT_MAX})")
    parser.add_argument("--rotate-penalty", type=int, default=ops.TRACK_ROT_PENALTY, metavar="P",
                        help=f"with --rotate: what a turn must win by, in 1/4096 grey levels per sample, "
                             f"0..{_lib.TRACK_MAX_SCALE_PENALTY} (default {ops.TRACK_ROT_PENALTY})")

    parser.add_argument("--reacquire", type=int, nargs="?", const=ops.TRACK_RELOST, default=None, metavar="RELOST",
                        help=f"look for a face that the search window lost in the whole frame, with the key box's own "
                             f"template, and take it from there at a mean absolute difference of at most RELOST grey "
                             f"levels, 0..255 (default {ops.TRACK_RELOST}, half of --lost's default: a whole frame has far "
                             f"more candidates than the window); not with --scale or --rotate")

    args = parser.parse_args(argv)
    try:
        check_settings(sorted_keys(args.key), args.batch_frames, args.search, args.adapt, args.lost, args.template_side,
                       args.scale, args.scale_penalty, args.rotate, args.rotate_step, args.rotate_max, args.rotate_penalty,
                       sorted_key_angles(args.key_angle), args.reacquire)
    except ValueError as e:
        parser.error(str(e))
    return args


def sorted_keys(keys):
    """keys: (k, x, y, w, h) each -> {k: (x, y, w, h)} in the order of k; a ValueError for none, a negative or a repeated
    frame index and a box without extent"""
    rows = sorted(tuple(int(v) for v in key) for key in keys or [])
    if not rows or any(len(row) != 5 for row in rows):
        raise ValueError("--key: at least one key `K X Y W H` is needed")
    out = {}
    for k, x, y, w, h in rows:
        if k < 0:
            raise ValueError(f"--key: frame index {k} is negative")
        if k in out:
            raise ValueError(f"--key: frame {k} has two keys")
        if w <= 0 or h <= 0:
            raise ValueError(f"--key: the box of frame {k} has extent {w} x {h}")
        out[k] = (x, y, w, h)
    return out


def sorted_key_angles(pairs):
    """pairs: (k, a) each, a in degrees -> {k: a in integer hundredths of a degree, wrapped to (-18000, 18000]} in the order
    of k, or None for no pair; a ValueError for a negative or a repeated frame index and an angle that is no finite number"""
    if not pairs:
        return None
    out = {}
    try:
        rows = sorted((int(k), ops.angle_hundredths(a)) for k, a in pairs)
    except (TypeError, ValueError):
        raise ValueError("--key-angle: `K A`, a frame index and an angle in decimal degrees") from None
    for k, a in rows:
        if k < 0:
            raise ValueError(f"--key-angle: frame index {k} is negative")
        if k in out:
            raise ValueError(f"--key-angle: frame {k} has two angles")
        out[k] = a
    return out


def interpolate_key_angles(key_angles, frames):
    """{k: hundredths} -> the angle of frames 0 .. frames - 1 in integer hundredths: linear between two keys (floor division),
    constant before the first key and after the last"""
    ks = list(key_angles)
    out = []
    for k in range(frames):
        if k <= ks[0]:
            out.append(key_angles[ks[0]])
        elif k >= ks[-1]:
            out.append(key_angles[ks[-1]])
        else:
            k1 = next(q for q in ks if q >= k)
            k0 = ks[ks.index(k1) - 1]
            a0, a1 = key_angles[k0], key_angles[k1]
            out.append(a0 + (a1 - a0) * (k - k0) // (k1 - k0))
    return out


def check_settings(keys, batch_frames, search, adapt, lost, template_side, scale=False,
                   scale_penalty=ops.TRACK_SCALE_PENALTY, rotate=False, rotate_step=ops.TRACK_ROT_STEP,
                   rotate_max=ops.TRACK_ROT_MAX, rotate_penalty=ops.TRACK_ROT_PENALTY, key_angles=None, reacquire=None):
    """keys: what `sorted_keys` gave; key_angles: what `sorted_key_angles` gave; reacquire: None, or the threshold relost.
    A ValueError for a setting out of range, --rotate with --scale, --reacquire with either, and with --rotate a step and
    range `ops.track_rot_table` refuses, a key angle at a frame without a key or beyond the range"""
    if int(batch_frames) < 1:
        raise ValueError("--batch-frames is at least 1")
    if not isinstance(scale, bool):
        raise ValueError(f"--scale is True or False, not {scale!r}")
    if not isinstance(rotate, bool):
        raise ValueError(f"--rotate is True or False, not {rotate!r}")
    if rotate and scale:
        raise ValueError("--rotate with --scale: the rotation search keeps the key's size, the two cannot be combined")
    if reacquire is not None:
        if isinstance(reacquire, bool) or not isinstance(reacquire, int) or not 0 <= reacquire <= 255:
            raise ValueError(f"--reacquire is an integer in 0..255, not {reacquire!r}")
        if scale or rotate:
            which = "--scale" if scale else "--rotate"
            kept = "a level" if scale else "an angle"
            raise ValueError(f"--reacquire with {which}: that search keeps {kept}, which a whole-frame search of one size and "
                             f"one angle cannot restore, the two cannot be combined")
    for name, value, low, high in (("--search", search, 1, _lib.TRACK_MAX_SEARCH), ("--adapt", adapt, 0, 8),
                                   ("--lost", lost, 0, 255),
                                   ("--template-side", template_side, _lib.TRACK_MIN_SIDE, _lib.TRACK_MAX_SIDE),
                                   ("--scale-penalty", scale_penalty, 0, _lib.TRACK_MAX_SCALE_PENALTY),
                                   ("--rotate-penalty", rotate_penalty, 0, _lib.TRACK_MAX_SCALE_PENALTY),
                                   ("--rotate-step", rotate_step, 1, 18000), ("--rotate-max", rotate_max, 0, 180)):
        if isinstance(value, bool) or not isinstance(value, int) or not low <= value <= high:
            raise ValueError(f"{name} is an integer in {low}..{high}, not {value!r}")
    if rotate:
        try:
            amax = len(ops.track_rot_table(rotate_step, rotate_max)) // 2
        except ValueError as e:
            raise ValueError(f"--rotate-step {rotate_step} with --rotate-max {rotate_max}: {e}") from None
        for k, a in (key_angles or {}).items():
            if k not in keys:
                raise ValueError(f"--key-angle: with --rotate the angle of frame {k} seeds the tracker, and frame {k} has no --key")
            if (2 * abs(a) + rotate_step) // (2 * rotate_step) > amax:
                raise ValueError(f"--key-angle: {a / 100.0:.2f} degrees at frame {k} is beyond --rotate-max {rotate_max}")
    return keys


def write_track(path, track, header=(), angles=None):
    """line k for frame k: `x y w h`, or `-` where track[k] is None, behind `# ` comment lines -- what ops.read_box_track
    parses.  angles (integer hundredths of a degree, one per frame): a fifth column in decimal degrees -- what
    ops.read_rbox_track parses"""
    with open(path, "w") as f:
        for line in header:
            f.write(f"# {line}\n")
        for k, box in enumerate(track):
            if box is None:
                f.write("-\n")
            elif angles is None:
                f.write("{} {} {} {}\n".format(*box))
            else:
                f.write("{} {} {} {} {:.2f}\n".format(*box, angles[k] / 100.0))


class TrackFaceBox():
    """keys: (k, x, y, w, h) each, the face box marked at frame k.  frames=: an iterable of decoded BGR frames instead of the
    video file (cv2 is not needed then); sink=: a callable that takes each frame's box, (x, y, w, h) or None -- without an
    output_path no file is written then.  .track holds the result, entry k for frame k: None before the first key and where
    the face was not found, the key's own box (clipped to the frame) at a key frame.  A batch is one upload, one device call
    (one more, and a seed, per key frame inside it) and one small copy back; the result does not depend on batch_frames.
    scale=True: the size of the box is searched too (ops.track_template_scale_u8), scale_penalty what a change of size must
    win by; every key sets the size anew.
    key_angles: (k, a) each, the head's roll in degrees at frame k: the file gains a fifth column, .angles holds it in integer
    hundredths of a degree (`interpolate_key_angles`); None: the file is the four-column one.
    rotate=True: the angle of the box is searched too (ops.track_template_rot_u8; not together with scale=True), rotate_step
    hundredths of a degree a step, within +-rotate_max degrees, rotate_penalty what a turn must win by.  The fifth column
    and .angles (0 where the track has None; the sink still takes x y w h) are then the tracked angle, a multiple of the step; a key angle seeds the
    angle at its key frame -- a frame without a key there is a ValueError -- and a key without one seeds angle 0: the
    tracked angle is then relative to that key frame's pose.
    reacquire: None, or the threshold relost in grey levels a sample (ops.TRACK_RELOST is the tool's default): a frame that
    the window does not find is looked for in the whole frame with the key's own template (ops.track_template_reacq_u8; not
    together with scale=True or rotate=True) and is an ordinary box in .track; .reacquired counts them, `summary()` is the
    line of counts."""

    def __init__(self, video_path, keys, output_path=None, batch_frames=8, frames=None, sink=None, device="cuda",
                 search=ops.TRACK_SEARCH, adapt=ops.TRACK_ADAPT, lost=ops.TRACK_LOST,
                 template_side=ops.TRACK_TEMPLATE_SIDE, scale=False, scale_penalty=ops.TRACK_SCALE_PENALTY, key_angles=None,
                 rotate=False, rotate_step=ops.TRACK_ROT_STEP, rotate_max=ops.TRACK_ROT_MAX,
                 rotate_penalty=ops.TRACK_ROT_PENALTY, reacquire=None):

        self.video_path = Path(video_path)
        self.keys = sorted_keys(keys)
        self.key_angles = sorted_key_angles(key_angles)
        self.keys = check_settings(self.keys, batch_frames, search, adapt, lost, template_side, scale, scale_penalty,
                                   rotate, rotate_step, rotate_max, rotate_penalty, self.key_angles, reacquire)
        self.reacquire = reacquire
        self.reacquired = 0
        self.batch_frames = int(batch_frames)
        self.frames = frames
        self.sink = sink
        self.device = device
        self.search, self.adapt, self.lost, self.template_side = search, adapt, lost, template_side
        self.scale, self.scale_penalty = scale, scale_penalty
        self.rotate, self.rotate_step, self.rotate_max, self.rotate_penalty = rotate, rotate_step, rotate_max, rotate_penalty
        self.angles = [] if rotate else None
        if output_path is not None:
            self.output_path = Path(output_path)
        elif sink is None:
            self.output_path = self.video_path.with_name(f"{self.video_path.stem}_track.txt")
        else:
            self.output_path = None
        self.track = []

        if frames is None:
            import_cv2()

        self.track_video()

        if not self.rotate and self.key_angles is not None:
            self.angles = interpolate_key_angles(self.key_angles, len(self.track))
        if self.output_path is not None:
            write_track(self.output_path, self.track, self.header(), self.angles)
        late = [k for k in self.keys if k >= len(self.track)]
        if late:
            raise ValueError(f"--key: frame {late[0]} is past the video's last frame, {len(self.track) - 1}")

    def header(self):
        keys = ", ".join("{} {} {} {} {}".format(k, *box) for k, box in self.keys.items())
        lines = (f"track_face_box {self.video_path.name}: x y w h per frame, - where the face was not found",
                 f"keys (frame x y w h): {keys}",
                 f"search {self.search}, adapt {self.adapt}, lost {self.lost}, template side {self.template_side}")
        if self.scale:
            lines += (f"scale search: one level a frame, penalty {self.scale_penalty}",)
        if self.rotate:
            lines += (f"rotation search: one step of {self.rotate_step / 100.0:.2f} degrees a frame within +-{self.rotate_max}, "
                      f"penalty {self.rotate_penalty}; fifth column: the box's angle in degrees",)
            if self.key_angles is not None:
                angles = ", ".join(f"{k} {a / 100.0:.2f}" for k, a in self.key_angles.items())
                lines += (f"key angles (frame angle): {angles}",)
        elif self.key_angles is not None:
            angles = ", ".join(f"{k} {a / 100.0:.2f}" for k, a in self.key_angles.items())
            lines += (f"fifth column: the box's angle in degrees, interpolated between the key angles (frame angle): {angles}",)
        if self.reacquire is not None:
            lines += (f"re-acquisition: a frame the window loses is taken from a whole-frame search of the key's template at "
                      f"a cost of at most {self.reacquire} a sample",)
        return lines

    def summary(self):
        """the counts of the run in one line: found (by the window, the key frames among them), re-acquired, lost (written as
        `-`, the frames before the first key among them)"""
        lost = sum(box is None for box in self.track)
        return (f"{len(self.track)} frames: {len(self.track) - lost - self.reacquired} found, {self.reacquired} re-acquired, "
                f"{lost} lost")

    def track_video(self):

        frames = self.frames if self.frames is not None else open_video_as_generator(self.video_path)
        state = None

        for batch, real_frames in batches(frames, self.batch_frames):
            first = len(self.track)
            if state is None and not any(first <= k < first + real_frames for k in self.keys):
                boxes = [None] * real_frames  # before the first key: nothing to follow, nothing to upload
            else:
                if state is None:
                    state = ops.TrackState(self.device)
                boxes = self.track_batch(torch.from_numpy(batch).to(self.device)[:real_frames], first, state)
            for box in boxes:
                if self.rotate:  # (x, y, w, h, hundredths): the track stays x y w h, the angle goes beside it
                    self.angles.append(0 if box is None else box[4])
                    box = None if box is None else box[:4]
                self.track.append(box)
                if self.sink is not None:
                    self.sink(box)

    def track_batch(self, dev, first, state):
        """the boxes of the frames `dev` [n, h, w, 3] on the device, frame `first` of the video onwards: the stretches
        between key frames are followed, every key frame seeds"""
        n = len(dev)
        cuts = [i for i in range(n) if first + i in self.keys]
        boxes = [None] * n
        parts = []  # (index of the first frame, its device rows, the geometry they are in)
        start = 0
        for cut in cuts + [n]:
            if cut > start and state.seeded:
                parts.append((start, self.follow(dev[start:cut], state), state.geometry))
            if cut < n:
                if self.rotate:
                    angle = (self.key_angles or {}).get(first + cut, 0)
                    geometry = ops.track_seed(state, dev[cut], self.keys[first + cut], self.template_side, angle / 100.0,
                                              self.rotate_step, self.rotate_max)
                else:
                    geometry = ops.track_seed(state, dev[cut], self.keys[first + cut], self.template_side,
                                              reacquire=self.reacquire is not None)
                s, tx, ty, _, _, ox, oy, fw, fh = geometry
                boxes[cut] = (tx * s + ox, ty * s + oy, fw, fh)  # the key's box, clipped
                if self.rotate:  # and the angle of the seed's index
                    boxes[cut] += ((2 * abs(angle) + self.rotate_step) // (2 * self.rotate_step) * self.rotate_step
                                   * (1 if angle >= 0 else -1),)
            start = cut + 1
        if parts:
            rows = torch.cat([part[1] for part in parts]).cpu().tolist()  # one copy back
            at = 0
            for index, part, geometry in parts:
                count = len(part)
                if self.rotate:
                    boxes[index:index + count] = ops.track_rot_faces(rows[at:at + count], geometry, self.rotate_step)
                elif self.scale:
                    boxes[index:index + count] = ops.track_scale_faces(rows[at:at + count], geometry, dev.shape[1:3])
                else:
                    boxes[index:index + count] = ops.track_faces(rows[at:at + count], geometry)
                    self.reacquired += sum(int(row[3]) == 2 for row in rows[at:at + count])
                at += count
        return boxes

    def follow(self, dev, state):
        if self.rotate:
            return ops.track_template_rot_u8(dev, state, self.search, self.adapt, self.lost, 1, self.rotate_penalty,
                                             self.rotate_step, self.rotate_max)
        if self.scale:
            return ops.track_template_scale_u8(dev, state, self.search, self.adapt, self.lost, 1, self.scale_penalty)
        if self.reacquire is not None:
            return ops.track_template_reacq_u8(dev, state, self.search, self.adapt, self.lost, self.reacquire)
        return ops.track_template_u8(dev, state, self.search, self.adapt, self.lost)


if __name__ == "__main__":
    main()
