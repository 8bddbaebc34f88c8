// glh_sort_networks.h -- the sorting networks of the velocity field's neighbour test (glh_velocity.hip: k_vf_test): the
// 8 neighbours of a node at radius 1 and the 24 at radius 2 are sorted in registers, which takes compare-exchanges with
// compile-time indices only (glh_median.h says why: runtime-indexed register arrays go to scratch on gfx950).
//
// Both are Batcher's odd-even merge sort: the 8-wire network as it is (19 exchanges), the 24-wire one the 32-wire network
// without every exchange that touches a wire from 24 on (132 of 191 are left).  The pruning is sound because every
// exchange X(a, b) has a < b and leaves the minimum on a: with +inf on the wires from 24 on, an exchange that reaches
// one of them changes nothing.  Comparator count is no goal here.  The lists are X-macros so that
// tests/test_velocity_field.py can parse them and prove them with the 0/1 principle over all 2^8 and 2^24 binary inputs.
#pragma once

// clang-format off
#define GLH_SORT8_NETWORK(X) \
  X(0,1) X(2,3) X(0,2) X(1,3) X(1,2) X(4,5) X(6,7) X(4,6) X(5,7) X(5,6) \
  X(0,4) X(2,6) X(2,4) X(1,5) X(3,7) X(3,5) X(1,2) X(3,4) X(5,6)

#define GLH_SORT24_NETWORK(X) \
  X(0,1) X(2,3) X(0,2) X(1,3) X(1,2) X(4,5) X(6,7) X(4,6) X(5,7) X(5,6) \
  X(0,4) X(2,6) X(2,4) X(1,5) X(3,7) X(3,5) X(1,2) X(3,4) X(5,6) X(8,9) \
  X(10,11) X(8,10) X(9,11) X(9,10) X(12,13) X(14,15) X(12,14) X(13,15) X(13,14) X(8,12) \
  X(10,14) X(10,12) X(9,13) X(11,15) X(11,13) X(9,10) X(11,12) X(13,14) X(0,8) X(4,12) \
  X(4,8) X(2,10) X(6,14) X(6,10) X(2,4) X(6,8) X(10,12) X(1,9) X(5,13) X(5,9) \
  X(3,11) X(7,15) X(7,11) X(3,5) X(7,9) X(11,13) X(1,2) X(3,4) X(5,6) X(7,8) \
  X(9,10) X(11,12) X(13,14) X(16,17) X(18,19) X(16,18) X(17,19) X(17,18) X(20,21) X(22,23) \
  X(20,22) X(21,23) X(21,22) X(16,20) X(18,22) X(18,20) X(17,21) X(19,23) X(19,21) X(17,18) \
  X(19,20) X(21,22) X(18,20) X(19,21) X(17,18) X(19,20) X(21,22) X(0,16) X(8,16) X(4,20) \
  X(12,20) X(4,8) X(12,16) X(2,18) X(10,18) X(6,22) X(14,22) X(6,10) X(14,18) X(2,4) \
  X(6,8) X(10,12) X(14,16) X(18,20) X(1,17) X(9,17) X(5,21) X(13,21) X(5,9) X(13,17) \
  X(3,19) X(11,19) X(7,23) X(15,23) X(7,11) X(15,19) X(3,5) X(7,9) X(11,13) X(15,17) \
  X(19,21) X(1,2) X(3,4) X(5,6) X(7,8) X(9,10) X(11,12) X(13,14) X(15,16) X(17,18) \
  X(19,20) X(21,22)
// clang-format on
