"""Action labels for the SegmentEncoder's training (reference dataset/action_adapter.py): item i of the wrapped dataset plus

    action_label     the primitive's name: the text before the first ':' of item["info"][1]
    action_label_id  its index in ACTION_LIST
    action_onehot    (len(ACTION_LIST),) int32

ACTION_LIST is the reference's list of the 69 primitive names, in its order (the class ids of a trained checkpoint depend on it);
tests/golden/enctrain_action_list.txt holds the captured copy it is checked against."""
from __future__ import annotations

from typing import Dict

import numpy as np

ACTION_LIST = (
    "cap scoop pour wipe spread grip scrape rearrange press_button place_onto take_outside hold cut screw assemble stir unscrew "
    "trigger_lever open_gate place_inside close_gate uncap brush_whiteboard close_laptop_lid use_keyboard remove_usb remove_power_plug "
    "plug_in_power_plug insert_usb use_gamecontroller insert_lightbulb pull_out_drawer insert_pencil sharpen_pencil remove_pencil "
    "write_on_paper remove_lid put_on_lid shear_paper staple_paper_together remove_the_pen_cap write_on_whiteboard cap_the_pen "
    "put_flower_into_vase push_in_drawer remove_lightbulb open_laptop_lid open_book use_mouse remove_from_test_tube_rack hold_test_tube "
    "heat_test_tube place_test_tube_on_rack_with_holder pour_in_lab place_on_test_tube_rack put_off_alcohol_lamp shake_lab_container "
    "place_asbestos_mesh uncap_alcohol_lamp ignite_alcohol_lamp heat_beaker stir_experiment_substances remove_test_tube swap "
    "remove_test_tube_from_rack_with_holder flip_open_tooth_paste_cap squeeze_tooth_paste flip_close_tooth_paste_cap close_book"
).split()


class ActionRecognitionAdapter:
    def __init__(self, interaction_segment_dataset):
        self.interaction_segment_dataset = interaction_segment_dataset
        self.action_list = list(ACTION_LIST)
        self.max_action = len(self.action_list)

    def __getitem__(self, index: int) -> Dict:
        item = self.interaction_segment_dataset[index]
        label = str(item["info"][1].split(":")[0])
        label_id = self.action_list.index(label)  # (ValueError for a name outside the list, as the reference)
        onehot = np.zeros(self.max_action, dtype=np.int32)
        onehot[label_id] = 1
        item["action_label"], item["action_label_id"], item["action_onehot"] = label, label_id, onehot
        return item

    def __len__(self) -> int:
        return len(self.interaction_segment_dataset)
