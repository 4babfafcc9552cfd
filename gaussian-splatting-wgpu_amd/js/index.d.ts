// Type declarations for the Node host (the reference is TypeScript; no tsc is available offline,
// so these are hand-written and mirror src/renderer.ts, src/camera.ts, src/ply.ts).
export type Mat4 = Float32Array;
export type Vec3 = Float32Array;
export interface CanvasLike { width: number; height: number; manual?: boolean; onFrame?(rgba: Uint8Array, width: number, height: number): void; }
export interface CameraRaw { id: number; img_name: string; width: number; height: number; position: number[]; rotation: number[][]; fx: number; fy: number; }
export class Camera {
  height: number; width: number; viewMatrix: Mat4; perspective: Mat4; focalX: number; focalY: number; scaleModifier: number;
  constructor(height: number, width: number, viewMatrix: Mat4, perspective: Mat4, focalX: number, focalY: number, scaleModifier: number);
  static default(canvas?: CanvasLike): Camera;
  setScale(scale: number): void; setFocalX(f: number): void; setFocalY(f: number): void;
  getPosition(): Vec3; getProjMatrix(): Mat4;
  translate(x: number, y: number, z: number): void; rotate(x: number, y: number, z: number): void;
  packUniforms(canvasWidth: number, canvasHeight: number, out?: Float32Array): Float32Array;
}
export class InteractiveCamera {
  constructor(camera: Camera, canvas: CanvasLike);
  static default(canvas: CanvasLike): InteractiveCamera;
  key(k: string): boolean; drag(movementX: number, movementY: number): void; wheel(deltaY: number): void;
  setNewCamera(c: Camera): void; isDirty(): boolean; getCamera(): Camera;
}
export class PackedGaussians {
  numGaussians: number; sphericalHarmonicsDegree: number; readonly nShCoeffs: number;
  gaussianLayout: { size: number }; gaussianArrayLayout: { size: number }; gaussiansBuffer: ArrayBuffer;
  constructor(arrayBuffer: ArrayBuffer);
  static fromRecords(arrayBuffer: ArrayBuffer, numGaussians: number): PackedGaussians;
  static fromFile(path: string): PackedGaussians;
}
export class Renderer {
  canvas: CanvasLike; interactiveCamera: InteractiveCamera; numGaussians: number; tileSize: number; numIntersections: number; numFrames: number;
  constructor(canvas: CanvasLike, interactiveCamera: InteractiveCamera, device: number | { ordinal: number; flags?: number; shareWith?: Renderer }, gaussians: PackedGaussians, tileSize: number);
  animate(): Promise<void>; destroy(): Promise<void>;
  renderUniforms(uniforms: Float32Array, debug?: boolean): void; readPixels(): Uint8Array; readBuffer(which: number): ArrayBuffer;
  /** FLAG.AUX_OUTPUTS: the last frame's accumulated opacity, f32[height][slabWidth]. */
  readAlpha(): Float32Array;
  /** FLAG.AUX_OUTPUTS: the last frame's accumulated depth D, or D / alpha where alpha > 0 (else 0) with normalized = true. */
  readDepth(normalized?: boolean): Float32Array;
  /** gs_pick on the last frame: queries = x,y pairs of canvas pixels (at most 65536 pairs); the canonical (EXACT) blend's answer. */
  pick(queries: Uint32Array, maxContrib?: number): PickResult;
  /** Adds what the last frame shows of the region's canvas pixels (null: the whole canvas) to the per-splat coverage planes; returns the region's pixels in this renderer's slab. */
  accumulateCoverage(region?: CoverRegion | null): number;
  resetCoverage(): void;
  /** count records of 16 bytes (gs_coverage_rec); record i: u64[2 i] sumQ, u32[4 i + 2] hits, f32[4 i + 3] maxWeight (COVERAGE_FIELD holds the byte offsets). */
  readCoverage(): { count: number; bytes: ArrayBuffer; u64: BigUint64Array; u32: Uint32Array; f32: Float32Array };
  /** FLAG.SPLAT_STATE: applies op with bits to the splats that pass the where filter and for which (hits >= minHits && maxWeight >= minWeight) == covered; returns how many those are. */
  stateCoverage(filter: { minHits?: number; minWeight?: number; covered?: boolean; whereMask?: number; whereValue?: number }, op: number, bits: number): number;
  /** Splat attributes: one f32 per resident splat (attr.kind = ATTR.*; attr.p: the point of DIST2 or the plane of PLANE). */
  attrSummary(attr: SplatAttr, where?: { mask?: number; value?: number }): { matched: number; nan: number; min: number; max: number };
  attrHistogram(attr: SplatAttr, lo: number, hi: number, bins?: number, where?: { mask?: number; value?: number }): { counts: number[]; below: number; above: number; nan: number };
  attrValues(attr: SplatAttr, where?: { mask?: number; value?: number }, withIds?: boolean): { values: Float32Array; ids: Uint32Array | null };
  /** FLAG.SPLAT_STATE: op / bits on the splats that pass the where filter and for which (lo <= v <= hi) == inside; returns how many. */
  stateAttr(attr: SplatAttr, range: { lo?: number; hi?: number; inside?: boolean; whereMask?: number; whereValue?: number }, op: number, bits: number): number;
  /** Neighbourhoods: counts, for every splat passing the qry filter, the splats passing the src filter within radius (self excluded, <= inclusive), saturated at limit, into a resident u32 plane. Throws with code -8 beyond maxCandidates. */
  neighCount(opts: { radius: number; limit?: number; srcMask?: number; srcValue?: number; qryMask?: number; qryValue?: number; maxCandidates?: number }): { queried: number; sources: number; candidates: number; cells: number[]; cellEdge: number };
  /** The count plane in splat order. */
  neighRead(): Uint32Array;
  /** FLAG.SPLAT_STATE: op / bits on the splats that pass the where filter and whose count c has (minCount <= c <= maxCount) == inside; returns how many. */
  stateNeigh(opts: { minCount?: number; maxCount?: number; inside?: boolean; whereMask?: number; whereValue?: number }, op: number, bits: number): number;
  setOption(key: number, value: number): void;
  /** FLAG.SPLAT_STATE: applies op (STATE.SET / CLEAR / TOGGLE / ASSIGN) with bits to every splat whose centre lies in the region and whose byte passes the where filter; returns how many those are. */
  stateRegion(region: StateRegion, op: number, bits: number): number;
  stateIds(ids: Uint32Array, op: number, bits: number): void;
  stateCount(mask: number, value: number): number;
  /** The state plane as it is now, one byte per resident splat. */
  readState(): Uint8Array;
  writeState(bytes: Uint8Array): void;
  /** Indices of the splats with (s & mask) == value, ascending. */
  listState(mask: number, value: number): Uint32Array;
  /** The matching splats as 320-byte records (accepted by PackedGaussians.fromRecords, as an uploaded buffer is) and their indices; default every splat. */
  exportSplats(filter?: { mask?: number; value?: number }): { buffer: ArrayBuffer; ids: Uint32Array };
  /** Keeps the matching splats, drops the rest for good, renumbers; returns ids[new index] = old index and updates numGaussians. */
  compact(mask: number, value: number): Uint32Array;
  /** compact(STATE.HIDDEN, 0). */
  deleteHidden(): Uint32Array;
  /** Streams the matching splats into a binary 3DGS .ply; returns how many were written. */
  savePly(file: string, options?: { mask?: number; value?: number; shDegree?: number }): number;
  /** Applies what composeTransform returned, in place, to the resident splats with (s & mask) == value (default: the selection; (0, 0): every splat); returns how many those are. The next frame sees the moved splats; the inverse transform is not a bit-exact undo. */
  transformSplats(xform: ArrayBuffer | Float32Array, mask?: number, value?: number): number;
  stats(): { numGaussians: number; numVisible: number; numIntersections: number; numProcessed: number; numTiles: number; sortPasses: number; frames: number; frameUs: number; stageUs: number[]; numEvaluated: number; depthOrdered: number; tightBinning: number; graphFrames: number; capacity: number; maxIntersectionsSeen: number; truncatedFrames: number };
}
export interface StateRegion {
  kind: number; a?: number[]; b?: number[]; x0?: number; y0?: number; x1?: number; y1?: number;
  uniforms?: Float32Array; mask?: Uint8Array; whereMask?: number; whereValue?: number;
}
export interface CoverRegion { x0?: number; y0?: number; x1?: number; y1?: number; mask?: Uint8Array }
export interface SplatAttr { kind: number; p?: ArrayLike<number> }
export const ATTR: { POS_X: 0; POS_Y: 1; POS_Z: 2; OPACITY_LOGIT: 3; LOG_SCALE_MIN: 4; LOG_SCALE_MAX: 5; LOG_SCALE_SUM: 6; ANISOTROPY: 7; DC_R: 8; DC_G: 9;
                     DC_B: 10; DIST2: 11; PLANE: 12; COVER_HITS: 13; COVER_MAX_WEIGHT: 14; COVER_SUM: 15 };
export const COVERAGE: { REC_BYTES: 16 };
export const COVERAGE_FIELD: { sumQ: 0; hits: 8; maxWeight: 12 };
export const STATE: { HIDDEN: 0x1; SELECTED: 0x2; SET: 1; CLEAR: 2; TOGGLE: 3; ASSIGN: 4 };
export const REGION: { ALL: 0; SPHERE: 1; BOX: 2; SCREEN_RECT: 3; SCREEN_MASK: 4 };
export const OPT: { SELECT_TINT: 11 };
export interface PickRecord {
  status: number; listLength: number; hitCount: number; firstId: number; firstDepth: number; maxId: number; maxWeight: number;
  medianId: number; medianDepth: number; alpha: number; depthAcc: number; reserved: number; contrib?: { id: number; weight: number }[];
}
export class PickResult {
  readonly count: number; readonly maxContrib: number;
  /** count records of 48 bytes (gs_pick_result); u32 / f32 view the same bytes, word 12 q + PICK_FIELD.x. */
  readonly bytes: ArrayBuffer; readonly u32: Uint32Array; readonly f32: Float32Array;
  /** count * maxContrib records {id, weight}: contribId[2 i], contribWeight[2 i + 1]; null when maxContrib = 0. */
  readonly contribBytes: ArrayBuffer | null; readonly contribId: Uint32Array | null; readonly contribWeight: Float32Array | null;
  get(q: number): PickRecord;
}
export const PICK: { OK: 0; OUTSIDE_SLAB: 1; NONE: 0xFFFFFFFF; MAX_QUERIES: 65536; MAX_CONTRIB: 256 };
export const PICK_FIELD: { status: 0; listLength: 1; hitCount: 2; firstId: 3; firstDepth: 4; maxId: 5; maxWeight: 6; medianId: 7; medianDepth: 8;
                           alpha: 9; depthAcc: 10; reserved: 11 };
export function loadFileAsArrayBuffer(path: string): Promise<ArrayBuffer>;
export function cameraFromJSON(raw: CameraRaw, canvasW: number, canvasH: number): Camera;
export function loadCameraFile(path: string, canvas?: CanvasLike): { name: string; camera: Camera }[];
export function getProjectionMatrix(znear: number, zfar: number, fovX: number, fovY: number): Mat4;
export function focal2fov(focal: number, pixels: number): number;
/** The inverse of PackedGaussians.fromFile: writes the records as a binary 3DGS .ply of that SH degree. */
export function savePly(file: string, gaussians: PackedGaussians, shDegree?: number): void;
/** The opaque gs_xform of p' = scale R (p - pivot) + pivot + translation, R the rotation of the quaternion (r, x, y, z; any non-zero length); uniform scale > 0 only. No context, no GPU. */
export function composeTransform(transform?: { rotation?: number[]; translation?: number[]; scale?: number; pivot?: number[] }): ArrayBuffer;
export function writePPM(file: string, rgba: Uint8Array, width: number, height: number): void;
export const BUF: { TILE_COUNTS: 0; TILE_OFFSETS: 1; GAUSSIAN_DATA: 2; KEYS_UNSORTED: 3; VALUES_UNSORTED: 4; KEYS: 5; VALUES: 6; RANGES: 7; RGBA8: 8; RGB_F32: 9;
                    ALPHA_F32: 13; DEPTH_F32: 14; SPLAT_STATE: 15 };
export const FLAG: { EXACT_BLEND: 0x1; F32_TAP: 0x2; TIMING: 0x4; AUX_OUTPUTS: 0x8; SPLAT_STATE: 0x10 };
