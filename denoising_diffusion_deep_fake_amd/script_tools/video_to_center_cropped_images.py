"""Turn a video into centre-cropped, resized training images plus images.txt
(d3f/script_tools/video_to_center_cropped_images.py).  Crop and bicubic resize run on the device in batches
(ops.crop_resize_cubic_u8); JPEGs are written with PIL (BGR -> RGB), as dataset.image_dataset reads them."""
import argparse
from pathlib import Path

import torch

from .. import ops
from .video_writer_context_manager import batches, import_cv2, open_video_as_generator


def main():

    args = parse_command_line_arguments()

    VideoToImages(
        args.video_path,
        args.width,
        args.height,
        batch_frames=args.batch_frames,
        antialias=args.antialias,
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

    return parser.parse_args(argv)


class VideoToImages():
    """frames=: an iterable of decoded BGR frames instead of the video file (cv2 is not needed then); the output folder
    is still named after video_path.  antialias=True: ops.crop_resize_cubic_u8(..., antialias=True)"""

    def __init__(self, video_path, image_width, image_height, batch_frames=16, frames=None, device="cuda",
                 antialias=False):

        self.video_path = Path(video_path)
        self.image_width = int(image_width)
        self.image_height = int(image_height)
        self.batch_frames = int(batch_frames)
        if self.batch_frames < 1:
            raise ValueError("batch_frames is at least 1")
        self.frames = frames
        self.device = device
        self.antialias = bool(antialias)

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
            resized = self.resize_frames(batch)
            for frame in resized[:real_frames]:
                file_path_list.append(self.save_frame_to_disk(frame, len(file_path_list)))

        self.save_file_path_list(file_path_list)

    def resize_frames(self, batch):
        """[n, h, w, 3] host BGR frames -> [n, height, width, 3] host BGR frames, cropped at the centre and resized"""
        dev = torch.from_numpy(batch).to(self.device)
        return ops.crop_resize_cubic_u8(dev, (self.image_height, self.image_width),
                                        antialias=self.antialias).cpu().numpy()

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
