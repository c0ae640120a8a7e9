"""Turn a video into centre-cropped, resized training images plus images.txt
(d3f/script_tools/video_to_center_cropped_images.py).  Crop and bicubic resize run on the device in batches
(ops.crop_resize_cubic_u8); JPEGs are written with PIL (BGR -> RGB), as dataset.image_dataset reads them.
--track FILE cuts every frame at the box of a detector's track instead (ops.track_crop_box), exactly the boxes
put_video_through_fake_model --track crops and pastes at: the model then sees what it is later asked to replace."""
import argparse
from pathlib import Path

import torch

from .. import ops
from .video_writer_context_manager import (add_track_arguments, batches, check_track_arguments, import_cv2, load_rtrack,
                                           load_track, open_video_as_generator, track_rotate_setting, track_setting)


def main():

    args = parse_command_line_arguments()

    VideoToImages(
        args.video_path,
        args.width,
        args.height,
        batch_frames=args.batch_frames,
        antialias=args.antialias,
        track=args.track,
        track_margin=args.track_margin,
        track_smooth=args.track_smooth,
        track_rotate=args.track_rotate,
        )


def parse_command_line_arguments(argv=None):
    parser = argparse.ArgumentParser()

    parser.add_argument("video_path", help="path to the video")
    parser.add_argument("width", help="output image width")
    parser.add_argument("height", help="output image height")
    parser.add_argument("--batch-frames", type=int, default=16, help="frames per device call")
    parser.add_argument("--antialias", action="store_true",
                        help="resize with the antialiased bicubic filter (Pillow's); use it when the crop is several times "
                             "the image size, and render videos through the trained model with the same flag")

    add_track_arguments(parser)

    args = parser.parse_args(argv)
    check_track_arguments(parser, args)
    return args


class VideoToImages():
    """frames=: an iterable of decoded BGR frames instead of the video file (cv2 is not needed then); the output folder
    is still named after video_path.  antialias=True: ops.crop_resize_cubic_u8(..., antialias=True).
    track=FILE (or a list of (x, y, w, h) boxes; track_margin=M, track_smooth=N with it): frame k is cut at
    `ops.track_crop_box` of the track's entry k, the frame counter running across batches, as RenderFakeVideo(track=) does.
    track_rotate=True: the track's entries carry an angle (`ops.read_rbox_track`) and every box is turned by it about its
    centre (`ops.crop_resize_cubic_u8`, angles=); not with antialias=True"""

    track_rotate = False  # the track's entries are (x, y, w, h, a)

    def __init__(self, video_path, image_width, image_height, batch_frames=16, frames=None, device="cuda",
                 antialias=False, track=None, track_margin=None, track_smooth=None, track_rotate=False):

        self.video_path = Path(video_path)
        self.image_width = int(image_width)
        self.image_height = int(image_height)
        self.batch_frames = int(batch_frames)
        if self.batch_frames < 1:
            raise ValueError("batch_frames is at least 1")
        self.frames = frames
        self.device = device
        self.antialias = bool(antialias)
        self.track_margin, track_smooth = track_setting(track, track_margin, track_smooth)
        self.track_rotate = track_rotate_setting(track, track_rotate, self.antialias)
        if self.track_rotate:
            self.track = load_rtrack(track, track_smooth)
        else:
            self.track = None if track is None else load_track(track, self.track_margin, track_smooth)
        self.frame_index = 0  # of the next batch's first frame: the track is followed across batches

        if frames is None:
            import_cv2()  # fail before the output folder is made

        self.create_output_folder()

        self.convert_video_to_images()

    def create_output_folder(self):

        output_dir_name = f"{self.video_path.stem}_w{self.image_width}_h{self.image_height}"
        self.output_dir_path = self.video_path.parent / output_dir_name
        self.output_dir_path.mkdir(exist_ok=True)

    def convert_video_to_images(self):

        file_path_list = []
        frames = self.frames if self.frames is not None else open_video_as_generator(self.video_path)

        for batch, real_frames in batches(frames, self.batch_frames):
            resized = self.resize_frames(batch, real_frames)
            for frame in resized[:real_frames]:
                file_path_list.append(self.save_frame_to_disk(frame, len(file_path_list)))

        self.save_file_path_list(file_path_list)

    def resize_frames(self, batch, real_frames=None):
        """[n, h, w, 3] host BGR frames -> [n, height, width, 3] host BGR frames, cropped at the centre -- with a track, each
        at its own box (the first real_frames of the batch are frames of the video, the rest padding) -- and resized"""
        dev = torch.from_numpy(batch).to(self.device)
        boxes = angles = None
        if self.track is not None:
            real = len(batch) if real_frames is None else real_frames
            h, w = batch.shape[1:3]
            geometry = (self.track, self.frame_index, real, h, w, self.image_width, self.image_height, self.track_margin)
            if self.track_rotate:
                boxes, angles = ops.track_crop_rboxes(*geometry)
                angles += [angles[-1]] * (len(batch) - real)
            else:
                boxes = ops.track_crop_boxes(*geometry)
            self.frame_index += real
            boxes += [boxes[-1]] * (len(batch) - real)
        return ops.crop_resize_cubic_u8(dev, (self.image_height, self.image_width), antialias=self.antialias,
                                        boxes=boxes, angles=angles).cpu().numpy()

    def save_frame_to_disk(self, frame, frame_index):
        from PIL import Image

        file_name = f"{frame_index:06}.jpg"

        file_path = self.output_dir_path / file_name

        Image.fromarray(frame[:, :, ::-1].copy()).save(file_path)  # BGR -> RGB

        return file_path

    def save_file_path_list(self, file_path_list):

        text_path = self.output_dir_path / "images.txt"

        with open(text_path, "w") as f:

            for file_path in file_path_list:

                relative_file_path = file_path.relative_to(self.output_dir_path)

                f.write(str(relative_file_path))
                f.write("\n")


if __name__ == "__main__":
    main()
