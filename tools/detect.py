"""Detect on paired RGB + IR images: the command-line form of the reference's detect_twostream.py.

    python tools/detect.py --weights W.pt --source1 RGB_DIR --source2 IR_DIR [--img-size 640] [--conf-thres 0.4] [--batch-size 8]
                           [--save-txt] [--save-conf] [--save-crop] [--nosave] [--hide-labels] [--line-thickness 2] ...

The options and their defaults are the reference's (detect_twostream.py:198-221) plus ``--batch-size`` and ``--device-jpeg`` (saved
.jpg / .jpeg images are encoded on the GPU instead of by PIL, to the same bytes; other suffixes stay on PIL).  Results go to
``--project/--name`` (incremented): ``<stem>_rgb.<ext>`` / ``<stem>_ir.<ext>`` with the boxes drawn, ``labels/<stem>.txt``,
``crops/<class>/<stem>.jpg``.  ``--view-img``, ``--update``, ``--augment`` and webcam / stream / video sources raise."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import msod_amd  # noqa: E402,F401
from msod_amd.detect import detect, make_parser  # noqa: E402


def main(argv=None):
    parser = make_parser()
    parser.add_argument('--device-jpeg', action='store_true',
                        help='encode saved .jpg / .jpeg images on the GPU (colour, DCT, quantisation; Huffman coding on host threads): the bytes PIL writes')
    opt = parser.parse_args(argv)
    print(opt)
    with torch.no_grad():
        return detect(opt=opt)


if __name__ == "__main__":
    main()
