"""cv2.VideoWriter as a context manager (d3f/script_tools/video_writer_context_manager.py) and the matching reader.
cv2 is imported only when a file is opened: the frame path itself runs without it through the `frames=` / `sink=` hooks
of RenderFakeVideo and VideoToImages."""
from pathlib import Path

from .. import ops

NO_CV2 = ("OpenCV (cv2) is not installed, and it is only needed to decode / encode video files: pass decoded BGR frames "
          "through the frames= hook (an iterable of [h, w, 3] uint8 arrays) and take the output frames through the "
          "sink= hook (a callable per frame) instead")


def import_cv2():
    try:
        import cv2
    except ImportError as e:
        raise ImportError(NO_CV2) from e
    return cv2


class VideoWriter():

    def __init__(self, output_path, w, h, fps):
        self.output_path = output_path
        self.w = w
        self.h = h
        self.fps = fps

    def __enter__(self):
        cv2 = import_cv2()
        four_cc = cv2.VideoWriter_fourcc(*"mp4v")
        self.video_writer = cv2.VideoWriter(filename=self.output_path, fourcc=four_cc, fps=self.fps,
                                            frameSize=(self.w, self.h))
        return self.video_writer

    def __exit__(self, *args):
        self.video_writer.release()


def video_fps(video_path):
    cv2 = import_cv2()
    video_reader = cv2.VideoCapture(str(video_path.resolve()))
    fps = video_reader.get(cv2.CAP_PROP_FPS)
    video_reader.release()
    return fps


def open_video_as_generator(video_path):
    """decoded BGR frames of a video file, one [h, w, 3] uint8 array at a time"""
    cv2 = import_cv2()
    video_reader = cv2.VideoCapture(str(video_path.resolve()))
    try:
        while video_reader.isOpened():
            frame_ok, frame = video_reader.read()
            if not frame_ok:
                break
            yield frame
    finally:
        video_reader.release()


def batches(frames, n):
    """(stacked [n, h, w, 3] batch, number of real frames in it): frames n at a time; a short last batch is padded by
    repeating its last frame, so every batch has the shape the first one planned (and captured) for"""
    import numpy as np
    chunk = []
    for frame in frames:
        chunk.append(np.asarray(frame))
        if len(chunk) == n:
            yield np.stack(chunk), n
            chunk = []
    if chunk:
        real = len(chunk)
        chunk += [chunk[-1]] * (n - real)
        yield np.stack(chunk), real


# ---- --track: the three flags of both tools that cut crops from a video ----
def add_track_arguments(parser):
    """--track, --track-margin, --track-smooth: the same three flags on both tools that cut crops from a video"""
    parser.add_argument("--track", default=None, metavar="FILE",
                        help="follow a detector's face boxes instead of the centre crop: a text file, line k for frame k, "
                             "`x y w h` in pixels (blanks or commas), `-` for no detection, # comments")
    parser.add_argument("--track-margin", type=float, default=None, metavar="M",
                        help=f"--track: the crop is M times the face box (default {ops.TRACK_MARGIN})")
    parser.add_argument("--track-smooth", type=int, default=None, metavar="N",
                        help="--track: average the track over 2 N + 1 frames against detector jitter (default 0: off)")
    parser.add_argument("--track-rotate", action="store_true",
                        help="--track: a line may carry a fifth field, the box's angle in decimal degrees (positive turns "
                             "the box clockwise on the screen; missing: 0), and every crop box is turned by it about its "
                             "centre; not with --antialias or --blend multiband")


def check_track_arguments(parser, args):
    try:
        track_setting(args.track, args.track_margin, args.track_smooth)
        track_rotate_setting(args.track, args.track_rotate, args.antialias, getattr(args, "blend", None))
    except ValueError as e:
        parser.error(str(e))


def track_rotate_setting(track, rotate, antialias, blend=None):
    """track_rotate= / --track-rotate, checked against what a rotated box does not have -> bool"""
    if not rotate:
        return False
    if track is None:
        raise ValueError("--track-rotate needs --track")
    if antialias:
        raise ValueError("--track-rotate with --antialias: the antialiased crop of a rotated box is out of scope")
    if blend == "multiband":
        raise ValueError("--track-rotate with --blend multiband: the multiband pyramid of a rotated box is out of scope")
    return True


def track_setting(track, margin, smooth):
    """the three track arguments, checked -> (margin, smooth) with the defaults filled in"""
    if track is None:
        if margin is not None:
            raise ValueError("--track-margin needs --track")
        if smooth is not None:
            raise ValueError("--track-smooth needs --track")
    margin = ops.TRACK_MARGIN if margin is None else float(margin)
    smooth = 0 if smooth is None else int(smooth)
    if not margin > 0:
        raise ValueError(f"--track-margin {margin} is not positive")
    if smooth < 0:
        raise ValueError(f"--track-smooth {smooth} is negative")
    return margin, smooth


def load_rtrack(track, smooth):
    """track: a track file's path with an optional fifth field, or the entries themselves (a list of (x, y, w, h) or
    (x, y, w, h, a), a in degrees) -> the smoothed track of (x, y, w, h, a)"""
    if isinstance(track, (str, Path)):
        faces = ops.read_rbox_track(track)
    else:
        faces = [tuple(int(v) for v in f[:4]) + (ops.angle_hundredths(f[4]) / 100.0 if len(f) > 4 else 0.0,) for f in track]
    if not faces:
        raise ValueError("track: no detection in the track")
    return ops.smooth_rbox_track(faces, smooth)


def load_track(track, margin, smooth):
    """track: a track file's path, or the boxes themselves (a list of (x, y, w, h)) -> the smoothed track"""
    faces = ops.read_box_track(track) if isinstance(track, (str, Path)) else [tuple(int(v) for v in f) for f in track]
    if not faces:
        raise ValueError("track: no detection in the track")
    return ops.smooth_box_track(faces, smooth)
