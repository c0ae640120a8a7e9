"""Render a video through a trained face-swap model as real|fake frames side by side
(d3f/script_tools/put_video_through_fake_model.py).  Per frame the reference crops at the centre, cv2.resize()s,
predicts and concatenates on the host; here all of that is one device call per batch of frames
(LitModule.predict_fake_frames -> Unet.predict_frames_u8), and cv2 only decodes and encodes.
--output full writes the swapped video instead: the source's frames at their own size with the fake pasted back into
the centre-crop box (LitModule.predict_fake_frames_full -> Unet.predict_frames_full_u8), still one device call per batch.
--track FILE follows a detector's per-frame face boxes instead of the centre crop (ops.read_box_track, ops.track_crop_box):
every frame is cropped, and with --output full pasted, at its own box; video_to_center_cropped_images cuts the training
images from the same track the same way."""
import argparse
import datetime
from contextlib import ExitStack, nullcontext
from pathlib import Path

from .. import ops
from .._lib import MULTIBAND_MAX_LEVELS, TEMPORAL_STRENGTH, TEMPORAL_THRESHOLD, temporal_setting
from ..train_deep_fake.lit_module import LitModule
from .video_writer_context_manager import (VideoWriter, add_track_arguments, batches, check_track_arguments, import_cv2,
                                           load_rtrack, load_track, open_video_as_generator, track_rotate_setting,
                                           track_setting, video_fps)


def main():

    args = parse_command_line_arguments()

    RenderFakeVideo(
        args.video_path,
        args.checkpoint_path,
        args.model_a_or_b,
        args.width,
        args.height,
        batch_frames=args.batch_frames,
        output=args.output,
        feather=args.feather,
        antialias=args.antialias,
        color_match=args.color_match,
        temporal=args.temporal,
        temporal_threshold=args.temporal_threshold,
        blend=args.blend,
        blend_levels=args.blend_levels,
        track=args.track,
        track_margin=args.track_margin,
        track_smooth=args.track_smooth,
        track_rotate=args.track_rotate,
        )


OUTPUTS = ("pair", "full")
COLOR_MATCHES = ("none", "meanstd")
BLENDS = ("feather", "multiband")


def parse_command_line_arguments(argv=None):
    parser = argparse.ArgumentParser()

    parser.add_argument("video_path", help="Video file you want to fake")
    parser.add_argument("checkpoint_path", help="Model checkpoint path")
    parser.add_argument("model_a_or_b", choices=["a", "b"], help="Use model A or B to fake image")
    parser.add_argument("width", help="desired video width")
    parser.add_argument("height", help="desired video height")
    parser.add_argument("--batch-frames", type=int, default=1, help="frames per device call")
    parser.add_argument("--output", choices=list(OUTPUTS), default="pair",
                        help="pair: real|fake centre crops side by side at the network's size; full: the source's frames "
                             "at their own size with the fake pasted back into the crop box")
    parser.add_argument("--feather", type=int, default=None,
                        help="--output full: width in source pixels of the ramp over which the fake fades into the frame "
                             "(default: min(crop_w, crop_h) // 16)")
    parser.add_argument("--antialias", action="store_true",
                        help="resize the crop with the antialiased bicubic filter (Pillow's); use it when the crop is "
                             "several times the network's size, and on a model whose training images were made with it")

    parser.add_argument("--color-match", choices=list(COLOR_MATCHES), default=None,
                        help="--output full: match the fake's colour to the crop it replaces before the paste; meanstd: "
                             "mean and standard deviation per frame and channel (default: none)")

    parser.add_argument("--temporal", type=float, nargs="?", const=TEMPORAL_STRENGTH, default=None, metavar="STRENGTH",
                        help="filter the fake against flicker, in either output: where the crop stands still the fake is "
                             "averaged over time with this strength in (0, 1), where it moves the network's bytes pass "
                             f"(bare flag: {TEMPORAL_STRENGTH}; default: off)")
    parser.add_argument("--temporal-threshold", type=int, default=None, metavar="N",
                        help="--temporal: mean absolute change of the crop, in levels per sample over a pixel's 3 x 3 "
                             f"surroundings, from which a pixel counts as moving (1..255, default {TEMPORAL_THRESHOLD})")

    parser.add_argument("--blend", choices=list(BLENDS), default=None,
                        help="--output full: how the fake fades into the frame; feather: one ramp of --feather pixels; "
                             "multiband: low frequencies fade over --feather pixels, fine detail over a fraction of it, so "
                             "that a wide ramp hides the brightness step without ghosting edges (default: feather)")
    parser.add_argument("--blend-levels", type=int, default=None, metavar="N",
                        help=f"--blend multiband: frequency bands of the blend (1..{MULTIBAND_MAX_LEVELS}; every crop box "
                             "must be at least 2^N pixels on its short side; default: from the feather)")

    add_track_arguments(parser)

    args = parser.parse_args(argv)
    check_track_arguments(parser, args)
    if args.temporal_threshold is not None and args.temporal is None:
        parser.error("--temporal-threshold needs --temporal")
    try:
        temporal_setting(args.temporal, args.temporal_threshold)
    except ValueError as e:
        parser.error(str(e))
    if args.color_match is not None and args.output != "full":
        parser.error("--color-match needs --output full: the real|fake pair is not pasted anywhere")
    if args.blend == "multiband" and args.output != "full":
        parser.error("--blend multiband needs --output full: the real|fake pair is not pasted anywhere")
    if args.blend_levels is not None and args.blend != "multiband":
        parser.error("--blend-levels needs --blend multiband")
    if args.blend_levels is not None and not 1 <= args.blend_levels <= MULTIBAND_MAX_LEVELS:
        parser.error(f"--blend-levels is an integer in 1..{MULTIBAND_MAX_LEVELS}, not {args.blend_levels}")
    return args


class RenderFakeVideo():
    """frames=: an iterable of decoded BGR frames instead of the video file; sink=: a callable that takes each real|fake
    frame (output="full": each full frame) instead of the .mp4 writer; model=: a loaded LitModule instead of the
    checkpoint.  With both hooks no video file is touched and cv2 is not needed.
    output="full" takes the writer's size from the first frame, so the writer is opened when the first batch arrives: a
    source without frames leaves no output file (output="pair" knows its size up front and leaves an empty video).
    antialias=True: the crop is resized to the network's size with the antialiased bicubic filter, in either output.
    color_match="meanstd" (output="full" only): the fake's mean and standard deviation are matched to those of the crop it
    replaces, per frame and channel, before the paste; None / "none": the fake is pasted as the network made it.
    temporal=STRENGTH (either output; temporal_threshold=N with it): the fake is filtered against flicker along the video
    (`Unet.predict_frames_u8`, temporal=); the model's filter state is reset once, before the first batch.
    blend="multiband" (output="full" only; blend_levels=N in 1..6 with it): the fake is blended in per frequency band
    (`ops.paste_multiband_u8`) instead of over the single ramp; None / "feather": the ramp.  With a track and no
    blend_levels the levels come from the feather `track_feather` gives, and every box of the track is checked against
    2 ** N once, before the first batch.
    track=FILE (or a list of (x, y, w, h) boxes; track_margin=M, track_smooth=N with it): frame k is cropped, and with
    output="full" pasted, at `ops.track_crop_box` of the track's entry k instead of the centre box; the frame counter runs
    across batches, and the padding frames of a short last batch repeat the last real frame's box.  output="full" without
    feather= takes `ops.default_feather` of the smallest box of the whole track once, so the ramp does not change from
    batch to batch.  A tracked call runs eager (`Unet.predict_frames_u8`, boxes=).
    track_rotate=True: the track's entries carry an angle in degrees (`ops.read_rbox_track`; a list's entries may be
    (x, y, w, h, a)) and every box is turned by it about its centre, in the crop and in the paste
    (`Unet.predict_frames_u8`, angles=); the padding frames repeat the last real frame's angle too.  Not with antialias=True or
    blend="multiband"."""

    def __init__(self, video_path, checkpoint_path, model_a_or_b, image_width, image_height, batch_frames=1,
                 frames=None, sink=None, model=None, output="pair", feather=None, antialias=False, color_match=None,
                 temporal=None, temporal_threshold=None, track=None, track_margin=None, track_smooth=None, blend=None,
                 blend_levels=None, track_rotate=False):

        self.video_path = Path(video_path)
        self.checkpoint_path = Path(checkpoint_path) if checkpoint_path is not None else None
        self.model_a_or_b = model_a_or_b
        self.image_width = int(image_width)
        self.image_height = int(image_height)
        self.batch_frames = int(batch_frames)
        if self.batch_frames < 1:
            raise ValueError("batch_frames is at least 1")
        if output not in OUTPUTS:
            raise ValueError(f"output is one of {OUTPUTS}, not {output!r}")
        self.output = output
        self.feather = None if feather is None else int(feather)
        self.antialias = bool(antialias)
        if not (color_match is None or isinstance(color_match, str)) or color_match not in (None,) + COLOR_MATCHES:
            raise ValueError(f"color_match is None or one of {COLOR_MATCHES}, not {color_match!r}")
        if color_match is not None and output != "full":
            raise ValueError("color_match needs output='full': the real|fake pair is not pasted anywhere")
        self.color_match = color_match
        if temporal_threshold is not None and temporal is None:
            raise ValueError("temporal_threshold needs temporal")
        strength, threshold = temporal_setting(temporal, temporal_threshold)
        self.temporal = None if temporal is None or strength == 0.0 else (strength, threshold)
        if not (blend is None or isinstance(blend, str)) or blend not in (None,) + BLENDS:
            raise ValueError(f"blend is None or one of {BLENDS}, not {blend!r}")
        if blend == "multiband" and output != "full":
            raise ValueError("blend='multiband' needs output='full': the real|fake pair is not pasted anywhere")
        if blend_levels is not None and blend != "multiband":
            raise ValueError("blend_levels needs blend='multiband'")
        if blend_levels is not None and (isinstance(blend_levels, bool) or not isinstance(blend_levels, int)
                                         or not 1 <= blend_levels <= MULTIBAND_MAX_LEVELS):
            raise ValueError(f"blend_levels is an integer in 1..{MULTIBAND_MAX_LEVELS}, not {blend_levels!r}")
        self.blend = blend
        self.blend_levels = blend_levels
        self.track_margin, track_smooth = track_setting(track, track_margin, track_smooth)
        self.track_rotate = track_rotate_setting(track, track_rotate, self.antialias, blend)
        if self.track_rotate:
            self.track = load_rtrack(track, track_smooth)
        else:
            self.track = None if track is None else load_track(track, self.track_margin, track_smooth)
        self.frame_index = 0  # of the next batch's first frame: the track is followed across batches
        self.frames = frames
        self.sink = sink

        if frames is None or sink is None:
            import_cv2()  # a video file is read or written: fail before the checkpoint is loaded

        self.model = model if model is not None else self.load_model_from_checkpoint()

        if self.temporal is not None:
            self.model.reset_frame_temporal(self.model_a_or_b)  # this video does not follow the last one

        if self.output == "full":
            self.render_full_video()
        else:
            self.render_real_fake_video()

    def load_model_from_checkpoint(self):
        model = LitModule.load_from_checkpoint(self.checkpoint_path)
        model.cuda()
        model.eval()
        return model

    def batch_boxes(self, batch, real_frames):
        """(the boxes [B][4] of a batch of frames, or None without a track; their B angles, or None without track_rotate); the
        padding frames repeat the last real frame's"""
        if self.track is None:
            return None, None
        h, w = batch.shape[1:3]
        geometry = (self.track, self.frame_index, real_frames, h, w, self.image_width, self.image_height, self.track_margin)
        pad = len(batch) - real_frames
        self.frame_index += real_frames
        if self.track_rotate:
            boxes, angles = ops.track_crop_rboxes(*geometry)
            return boxes + [boxes[-1]] * pad, angles + [angles[-1]] * pad
        boxes = ops.track_crop_boxes(*geometry)
        return boxes + [boxes[-1]] * pad, None

    def whole_track_boxes(self, h, w):
        """the crop box of every entry of the track"""
        faces = [face[:4] for face in self.track]
        return ops.track_crop_boxes(faces, 0, len(faces), h, w, self.image_width, self.image_height, self.track_margin)

    def track_feather(self, h, w):
        """output="full" with a track and no feather=: `ops.default_feather` of the smallest box of the whole track"""
        boxes = self.whole_track_boxes(h, w)
        return ops.default_feather(min(b[2] for b in boxes), min(b[3] for b in boxes))

    def track_blend_levels(self, h, w, feather):
        """blend="multiband" with a track: the levels (blend_levels=, else `ops.multiband_levels` of the call's feather),
        after every box of the whole track has been checked against 2 ** levels"""
        levels = self.blend_levels if self.blend_levels is not None else ops.multiband_levels(feather)
        boxes = self.whole_track_boxes(h, w)
        for k, b in enumerate(boxes):
            if min(b[2], b[3]) < (1 << levels):
                raise ValueError(f"blend='multiband' with {levels} levels needs boxes of at least {1 << levels} pixels on "
                                 f"their short side; frame {k} of the track has {b[2]} x {b[3]}")
        return levels

    def render_real_fake_video(self):
        w = 2 * self.image_width
        h = self.image_height

        if self.sink is not None:
            writer = nullcontext(None)
        else:
            writer = VideoWriter(str(self.get_output_video_path()), w, h, self.get_input_video_properties())
        frames = self.frames if self.frames is not None else open_video_as_generator(self.video_path)

        with writer as video_writer:
            write = self.sink if self.sink is not None else video_writer.write
            for batch, real_frames in batches(frames, self.batch_frames):
                boxes, angles = self.batch_boxes(batch, real_frames)
                real_and_fake = self.model.predict_fake_frames(batch, self.model_a_or_b, self.image_width,
                                                               self.image_height, antialias=self.antialias,
                                                               temporal=self.temporal, boxes=boxes, angles=angles)
                for frame in real_and_fake[:real_frames]:  # the padding of a short last batch is dropped
                    write(frame)

    def render_full_video(self):
        frames = self.frames if self.frames is not None else open_video_as_generator(self.video_path)

        with ExitStack() as stack:
            write = self.sink
            feather = self.feather
            blend_levels = self.blend_levels
            track_checked = False
            for batch, real_frames in batches(frames, self.batch_frames):
                if feather is None and self.track is not None:
                    feather = self.track_feather(*batch.shape[1:3])
                if self.blend == "multiband" and self.track is not None and not track_checked:
                    blend_levels = self.track_blend_levels(*batch.shape[1:3], feather)
                    track_checked = True
                if write is None:  # the writer takes the source's size, read off the first frame
                    h, w = batch.shape[1:3]
                    write = stack.enter_context(VideoWriter(str(self.get_output_video_path("_full")), w, h,
                                                            self.get_input_video_properties())).write
                boxes, angles = self.batch_boxes(batch, real_frames)
                full = self.model.predict_fake_frames_full(batch, self.model_a_or_b, self.image_width,
                                                           self.image_height, feather=feather,
                                                           antialias=self.antialias, color_match=self.color_match,
                                                           temporal=self.temporal, boxes=boxes, angles=angles,
                                                           blend=self.blend, blend_levels=blend_levels)
                for frame in full[:real_frames]:  # the padding of a short last batch is dropped
                    write(frame)

    def get_output_video_path(self, tag=""):

        datetime_str = datetime.datetime.now().strftime("%Y%m%d_%a_%H%M%S")

        output_name = f"{self.video_path.stem}_model_{self.model_a_or_b}{tag}_{datetime_str}.mp4"
        output_path = self.video_path.with_name(output_name)
        return output_path

    def get_input_video_properties(self):
        return video_fps(self.video_path)


if __name__ == "__main__":
    main()
