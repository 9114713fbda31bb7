// k_form_end.inc -- the last line of a kernel text: forget what k_form.inc and the text defined, for the next form
#undef KNAME
#undef KFORM_PASTE
#undef KFORM_PASTE_
#undef KPREFIX
#undef KPOLICY_PARAM
#undef KEXPLORES
#undef KSIZES
#undef KRENEW_PARAM
#undef KFORM_PICK
#undef KPOLICY_FORMS
#undef KLOOKAHEAD_FORM
#undef KINDIVIDUAL_FORM
#undef KBASE
