'use strict';
// gsplat (Node host): the reference's class surface -- Renderer, Camera, InteractiveCamera,
// PackedGaussians, loadFileAsArrayBuffer -- backed by the MI355X-native C ABI through N-API.
const { Renderer, loadNative, savePly, composeTransform, PickResult, PICK, PICK_FIELD, STATE, REGION, COVERAGE, COVERAGE_FIELD } = require('./renderer');
const { Camera, InteractiveCamera, cameraFromJSON, loadCameraFile, getProjectionMatrix, focal2fov } = require('./camera');
const { PackedGaussians, loadFileAsArrayBuffer } = require('./ply');
const { mat4, mat3, vec3 } = require('./mat4');

// Writes an rgba8 frame as a binary PPM (presentation sink for hosts without a canvas).
function writePPM(file, rgba, width, height) {
  const fs = require('fs');
  const header = Buffer.from(`P6\n${width} ${height}\n255\n`, 'ascii');
  const rgb = Buffer.alloc(width * height * 3);
  for (let i = 0, j = 0; i < width * height; ++i) { rgb[j++] = rgba[4 * i]; rgb[j++] = rgba[4 * i + 1]; rgb[j++] = rgba[4 * i + 2]; }
  fs.writeFileSync(file, Buffer.concat([header, rgb]));
}

// the kinds of a splat attribute (gs_attr.kind): what attrSummary / attrHistogram / attrValues / stateAttr take as attr.kind
const ATTR = { POS_X: 0, POS_Y: 1, POS_Z: 2, OPACITY_LOGIT: 3, LOG_SCALE_MIN: 4, LOG_SCALE_MAX: 5, LOG_SCALE_SUM: 6, ANISOTROPY: 7, DC_R: 8, DC_G: 9,
               DC_B: 10, DIST2: 11, PLANE: 12, COVER_HITS: 13, COVER_MAX_WEIGHT: 14, COVER_SUM: 15 };

module.exports = {
  Renderer, Camera, InteractiveCamera, PackedGaussians, loadFileAsArrayBuffer, cameraFromJSON, loadCameraFile,
  getProjectionMatrix, focal2fov, mat4, mat3, vec3, writePPM, loadNative, savePly, composeTransform,
  BUF: { TILE_COUNTS: 0, TILE_OFFSETS: 1, GAUSSIAN_DATA: 2, KEYS_UNSORTED: 3, VALUES_UNSORTED: 4, KEYS: 5, VALUES: 6, RANGES: 7, RGBA8: 8, RGB_F32: 9,
         ALPHA_F32: 13, DEPTH_F32: 14, SPLAT_STATE: 15 },
  FLAG: { EXACT_BLEND: 0x1, F32_TAP: 0x2, TIMING: 0x4, AUX_OUTPUTS: 0x8, SPLAT_STATE: 0x10 },
  OPT: { SELECT_TINT: 11 },
  STATE, REGION, // STATE: { HIDDEN: 0x1, SELECTED: 0x2, SET: 1, CLEAR: 2, TOGGLE: 3, ASSIGN: 4 }; REGION: { ALL: 0, SPHERE: 1, BOX: 2, SCREEN_RECT: 3, SCREEN_MASK: 4 }
  ATTR,
  COVERAGE, COVERAGE_FIELD, // COVERAGE: { REC_BYTES: 16 }; COVERAGE_FIELD: { sumQ: 0, hits: 8, maxWeight: 12 } (byte offsets)
  PICK, PICK_FIELD, PickResult, // PICK: { OK: 0, OUTSIDE_SLAB: 1, NONE: 0xFFFFFFFF, MAX_QUERIES: 65536, MAX_CONTRIB: 256 }
};
