"""The reference's script tools (d3f/script_tools) around the device frame path: every step between a decoded BGR frame
and the frame that gets written runs on the GPU; only the video codec (cv2, optional) stays on the host.

    python -m d3f.script_tools.video_to_center_cropped_images <video> <width> <height>
    python -m d3f.script_tools.put_video_through_fake_model <video> <checkpoint> <a|b> <width> <height>
"""
