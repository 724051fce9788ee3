(ns raytrace-clj.gpu
  "GPU path for the render loop of raytrace-clj.core/-main (core.clj:100-108 of the reference).

  A scene built at the REPL from the reference's own records -- {:camera c :world w} as every
  make-* function of raytrace-clj.scene returns -- is flattened into the primitive arrays of
  include/rtmi.h and rendered by librtmi.so (HIP kernels for MI355X) through JNA.  Nothing is
  computed on the JVM; unknown record types raise ex-info {:unsupported-on-gpu-path ...} so the
  caller can fall back to the protocol path (raytrace-clj.core/pixel).

  STATUS: written blind (no JVM/lein/JNA jar in the build container); the Python mirror in
  raytrace_clj_amd/ exercises the same C-ABI call for call and is what the tests run.  What CAN be checked without a JVM is:
  tests/test_clj_conformance.py reads this file's (call-int \"rtmi_...\" ...) forms against the prototypes of include/rtmi.h --
  symbol, arity, (int ...) / (long ...) coercion of every scalar, element type of every array, handle vs handle-by-reference."
  (:require [clojure.core.matrix :as mat]
            [raytrace-clj.scene :as scene]
            [raytrace-clj.perlin :as perlin]
            [mikera.image.core :refer [new-image set-pixel save]]
            [mikera.image.colours :refer [rgb-from-components]])
  (:import [com.sun.jna Function Pointer Memory]
           [com.sun.jna.ptr PointerByReference]
           [raytrace_clj.hitable Hitlist bvh_node Sphere UVSphere MovingSphere RectXY RectXZ RectYZ Triangle
            FlipNormals Translate RotateY Box ConstantMedium]
           [raytrace_clj.shader Lambertian Metal Dielectric DiffuseLight Isotropic]
           [raytrace_clj.texture Constant UVGradient Checkerboard PerlinNoise PerlinTurbulence Marble
            FlipTextureU FlipTextureV ImageMap]
           [raytrace_clj.camera PinholeCamera ThinLensCamera]))

(mat/set-current-implementation :vectorz)

;;; ---------------------------------------------------------------------------------------------
;;; JNA plumbing: plain C functions, int return codes, rtmi_last_error for the text
;;; ---------------------------------------------------------------------------------------------

(def ^:private lib "rtmi")

(defn- cfn ^Function [name] (Function/getFunction lib name))

(defn- check [rc]
  (when-not (zero? rc)
    (throw (ex-info (str "rtmi error " rc ": "
                         (.invokeString (cfn "rtmi_last_error") (object-array 0) false))
                    {:rtmi-code rc}))))

(defn- call-int [name & args]
  (.invokeInt (cfn name) (object-array args)))

;;; ---------------------------------------------------------------------------------------------
;;; flattener: protocol extended onto the reference's records (field names as in the reference)
;;; ---------------------------------------------------------------------------------------------

(defn- v3 [v] [(mat/mget v 0) (mat/mget v 1) (mat/mget v 2)])

(def ^:private ^:dynamic *list-ctx* nil)   ; id of the Hitlist context being walked: the outermost Hitlist since the last bvh-node (nil outside any list)
(def ^:private ^:dynamic *slot* nil)       ; [identity of the list, position] of the list item being walked: a medium's LISTING
(def ^:private ^:dynamic *poisoned* false) ; a bvh-node INSIDE a Hitlist is among the ancestors: media below it cannot be expressed
(def ^:private list-ctxs (atom 0))         ; counts the Hitlist contexts of one flatten-scene walk
(def ^:private media-modes (atom #{}))   ; how flatten-scene's walk reached the media: :descent (bvh-nodes only above) / :hitlist (Hitlists only above)

(defprotocol GpuLeaves
  (leaves [this chain flip in-list? under-bvh?]
    "[{:leaf record :chain [[kind a b c] ...] :flip 0|1} ...] below this Hitable, in the order (and as often as) the
    reference's descent calls hit? on them; chain = the Translate / RotateY wrappers around the leaf, outermost first
    (kind 0 = translate offset.xyz, 1 = rotate-y sin cos 0).  A one-item make-bvh node holds the same child twice
    (hitable.clj:113-114) and is therefore listed twice: dedup-leaves drops the repeats for the primitive table, the
    repeats of ConstantMedium records are kept as the media call sequence.  in-list? / under-bvh?: a Hitlist / a bvh-node is among the
    ancestors -- a medium's hit? draws inside, so it matters whether its t-max comes narrowed by the siblings before it (Hitlist.hit?,
    hitable.clj:15-26: rtmi_scene_set_media_mode RTMI_MEDIA_HITLIST) or un-narrowed (bvh-node.hit?, hitable.clj:99-105); both at once is
    not supported."))

(defn- leaf [this chain flip] [{:leaf this :chain chain :flip flip :list *list-ctx*}])   ; :list -- which Hitlist context the entry stands in (its items are contiguous)

(extend-protocol GpuLeaves
  Hitlist      (leaves [this c f l b]                                                                      ; hitable.clj:15-26
                 ;; the items of a Hitlist (and of the Hitlists nested directly in it) see the closest hit of the items before them: one narrowing context
                 (binding [*list-ctx* (if (and l *list-ctx*) *list-ctx* (swap! list-ctxs inc))]
                   (doall (apply concat (map-indexed (fn [i it] (binding [*slot* [(System/identityHashCode this) i]] (doall (leaves it c f true b))))
                                                     (:items this))))))
  bvh_node     (leaves [this c f l b]                                                                      ; hitable.clj:97-105: both children, the un-narrowed interval
                 (binding [*list-ctx* nil *slot* nil *poisoned* (or *poisoned* (boolean l))]
                   (doall (concat (leaves (:left this) c f false true) (leaves (:right this) c f false true)))))
  Box          (leaves [this c f l b] (leaves (:sides this) c f l b))   ; hitable.clj:491-494: (hit? sides ...) with the caller's interval
  FlipNormals  (leaves [this c f l b] (leaves (:item this) c (bit-xor f 1) l b))                             ; hitable.clj:375-381
  Translate    (leaves [this c f l b] (leaves (:item this) (conj c (into [0.0] (v3 (:offset this)))) f l b)) ; hitable.clj:391-396
  RotateY      (leaves [this c f l b] (leaves (:obj this) (conj c [1.0 (:sin-theta this) (:cos-theta this) 0.0]) f l b)) ; :410-450
  ConstantMedium (leaves [this c f l b]                                                                      ; hitable.clj:516-541
                   (when *poisoned*
                     (throw (ex-info "a ConstantMedium below a bvh-node that itself sits inside a Hitlist is not supported on the GPU path"
                                     {:unsupported-on-gpu-path ConstantMedium})))
                   (swap! media-modes conj (cond (and l b) :narrowed l :hitlist :else :descent))
                   ;; inside a Hitlist WHERE a medium stands decides the t-max it is handed (hitable.clj:15-26): every LISTING of the record is a primitive of
                   ;; its own (:listing = the list item's slot: the same listing reached twice by the descent -- a one-item make-bvh -- is one primitive asked twice)
                   [{:leaf this :chain c :flip f :list *list-ctx* :listing (when l *slot*)}])
  Sphere       (leaves [this c f l b] (leaf this c f))
  UVSphere     (leaves [this c f l b] (leaf this c f))
  MovingSphere (leaves [this c f l b] (leaf this c f))
  RectXY       (leaves [this c f l b] (leaf this c f))
  RectXZ       (leaves [this c f l b] (leaf this c f))
  RectYZ       (leaves [this c f l b] (leaf this c f))
  Triangle     (leaves [this c f l b] (leaf this c f))
  Object       (leaves [this c f l b] (throw (ex-info (str (type this) " is not supported on the GPU path")
                                                      {:unsupported-on-gpu-path (type this)}))))

(defn- leaf-id-fn
  "object IDENTITY -> small integer (an IdentityHashMap, not System/identityHashCode: that is a 31-bit hash and two of the
  ~10 000 spheres of the cover scene at n = 50 collide with probability ~2 %)"
  []
  (let [ids (java.util.IdentityHashMap.)]
    (fn [leaf]
      (or (.get ids leaf)
          (let [k (.size ids)] (.put ids leaf k) k)))))

(defn- dedup-leaves
  "a one-item make-bvh stores the same child twice (hitable.clj:113-114): drop repeats of the same record under the
  same instance chain (the same record under two different instances is two primitives)"
  [lid xs]
  (let [seen (java.util.HashSet.)]
    (filterv #(.add seen [(lid (:leaf %)) (:chain %) (:flip %) (:listing %)]) xs)))

(defn- intern! [table obj build]
  ;; table: atom {:ids IdentityHashMap, :rows []}; children are interned first
  (let [^java.util.IdentityHashMap ids (:ids @table)]
    (or (.get ids obj)
        (let [row (build obj)
              id  (count (:rows @table))]
          (.put ids obj id)
          (swap! table update :rows conj row)
          id))))

(def ^:private images (atom []))   ; BufferedImages met while flattening, in ImageMap index order

(defn- pad12 [xs] (take 12 (concat (map double xs) (repeat 0.0))))

(defn- tex-row [textures t]
  (condp instance? t
    Constant     {:kind 0 :param (concat (v3 (:color t)) (repeat 9 0.0)) :child [-1 -1]}
    UVGradient   {:kind 1 :param (mapcat v3 [(:co t) (:cu t) (:cv t) (:cuv t)]) :child [-1 -1]}
    PerlinNoise      {:kind 3 :param (pad12 [(:scale t)]) :child [-1 -1]}                              ; texture.clj:60
    PerlinTurbulence {:kind 4 :param (pad12 [(:scale t) (:depth t)]) :child [-1 -1]}                   ; texture.clj:74
    Marble           {:kind 5 :param (pad12 [(:scale t) (:depth t)]) :child [-1 -1]}                   ; texture.clj:88
    FlipTextureU     {:kind 6 :param (pad12 []) :child [(intern! textures (:tex t) (partial tex-row textures)) -1]} ; :103
    FlipTextureV     {:kind 7 :param (pad12 []) :child [(intern! textures (:tex t) (partial tex-row textures)) -1]} ; :113
    ImageMap         (let [id (count @images)]                                                         ; texture.clj:126
                       (swap! images conj (:image t))
                       {:kind 8 :param (pad12 [id]) :child [-1 -1]})
    Checkerboard (let [c0 (intern! textures (:tex0 t) (partial tex-row textures))
                       c1 (intern! textures (:tex1 t) (partial tex-row textures))]
                   {:kind 2 :param (cons (double (:scale t)) (repeat 11 0.0)) :child [c0 c1]})
    (throw (ex-info (str (type t) " is not supported on the GPU path") {:unsupported-on-gpu-path (type t)}))))

(defn- mat-row [textures m]
  (let [tex (fn [t] (intern! textures t (partial tex-row textures)))]
    (condp instance? m
      Lambertian   {:kind 0 :tex (tex (:albedo m)) :param 0.0}
      Metal        {:kind 1 :tex (tex (:albedo m)) :param (double (:fuzz m))}
      Dielectric   {:kind 2 :tex -1 :param (double (:ri m))}
      DiffuseLight {:kind 3 :tex (tex (:tex m)) :param 0.0}
      Isotropic    {:kind 4 :tex (tex (:albedo m)) :param 0.0}                    ; shader.clj:129, a medium's phase function
      (throw (ex-info (str (type m) " is not supported on the GPU path") {:unsupported-on-gpu-path (type m)})))))

(defn- pad9 [xs] (take 9 (concat (map double xs) (repeat 0.0))))

(defn- prim-row [o]
  (condp instance? o
    MovingSphere {:kind 2 :geom (concat (v3 (:center0 o)) [(double (:radius o))] (v3 (:center1 o))
                                        [(double (:t0 o)) (double (:t1 o))])}
    UVSphere     {:kind 1 :geom (concat (v3 (:center o)) [(double (:radius o))] (v3 (:center o)) [0.0 1.0])}
    Sphere       {:kind 0 :geom (concat (v3 (:center o)) [(double (:radius o))] (v3 (:center o)) [0.0 1.0])}
    RectXY       {:kind 3 :geom (pad9 [(:x0 o) (:y0 o) (:x1 o) (:y1 o) (:k o)])}   ; hitable.clj:269
    RectXZ       {:kind 4 :geom (pad9 [(:x0 o) (:z0 o) (:x1 o) (:z1 o) (:k o)])}   ; hitable.clj:301
    RectYZ       {:kind 5 :geom (pad9 [(:y0 o) (:z0 o) (:y1 o) (:z1 o) (:k o)])}   ; hitable.clj:333
    Triangle     {:kind 6 :geom (concat (v3 (:v0 o)) (v3 (:v1 o)) (v3 (:v2 o)))}   ; hitable.clj:548
    ConstantMedium {:kind 7 :geom (pad9 [(:density o)])}))  ; hitable.clj:516; boundary range patched in by flatten-scene

(defn- camera-row [c]
  (condp instance? c
    ThinLensCamera {:kind 1 :cam (concat (mapcat v3 [(:origin c) (:lleft c) (:horiz c) (:vert c) (:u c) (:v c) (:w c)])
                                         [(double (:aperture c)) (double (:t0 c)) (double (:t1 c))])}
    PinholeCamera  {:kind 0 :cam (concat (mapcat v3 [(:origin c) (:lleft c) (:horiz c) (:vert c)]) (repeat 12 0.0))}
    (throw (ex-info (str (type c) " is not supported on the GPU path") {:unsupported-on-gpu-path (type c)}))))

(defn flatten-scene
  "{:camera c :world w} -> the flat arrays of include/rtmi.h (as Clojure primitive arrays)"
  [{:keys [camera world]}]
  (reset! images [])
  (reset! list-ctxs 0)
  (reset! media-modes #{})
  (let [called    (vec (leaves world [] 0 false false))    ; hit? invocation order, repeats included
        _         (when (> (count @media-modes) 1)
                    (throw (ex-info "media reached through a Hitlist and media reached through bvh-nodes only in one world: not supported on the GPU path"
                                    {:unsupported-on-gpu-path ConstantMedium})))
        lid       (leaf-id-fn)
        world-es  (dedup-leaves lid called)
        key-of    (fn [e] [(lid (:leaf e)) (:chain e) (:flip e) (:listing e)])
        index-of  (zipmap (map key-of world-es) (range))
        called-media (filterv #(instance? ConstantMedium (:leaf %)) called)
        media-calls (mapv #(index-of (key-of %)) called-media)
        ;; per call: the first primitive of the Hitlist items that narrow it (rtmi_scene_set_media_calls_narrowed); its own index: none (reached through bvh-nodes only)
        first-of  (reduce (fn [m [i e]] (if (and (:list e) (not (contains? m (:list e)))) (assoc m (:list e) i) m)) {} (map-indexed vector world-es))
        media-narrow-from (mapv (fn [e] (if (:listing e) (first-of (:list e)) (index-of (key-of e)))) called-media)
        ;; every medium's boundary is flattened on its own and appended AFTER the world (kind | 16)
        bounds    (reduce (fn [acc [i e]]
                            (if (instance? ConstantMedium (:leaf e))
                              (let [b (dedup-leaves (leaf-id-fn) (leaves (:boundary (:leaf e)) (:chain e) (:flip e) false false))]
                                (-> acc
                                    (assoc-in [:range i] [(+ (count world-es) (count (:prims acc))) (count b)])
                                    (update :prims into b)))
                              acc))
                          {:range {} :prims []}
                          (map-indexed vector world-es))
        n-world   (count world-es)
        entries   (into (vec world-es) (:prims bounds))
        prims     (mapv :leaf entries)
        material-of (fn [o] (if (instance? ConstantMedium o) (:phase-fn o) (:material o)))
        textures  (atom {:ids (java.util.IdentityHashMap.) :rows []})
        materials (atom {:ids (java.util.IdentityHashMap.) :rows []})
        prim-mat  (mapv #(intern! materials (material-of %) (partial mat-row textures)) prims)
        prows     (vec (map-indexed
                        (fn [i o]
                          (let [row (prim-row o)]
                            (cond
                              (instance? ConstantMedium o)
                              (let [[fb nb] (get-in bounds [:range i])]
                                (assoc row :geom (pad9 [(:density o) fb nb])))
                              (>= i n-world) (update row :kind bit-or 16)
                              :else row)))
                        prims))
        ;; transform table: every distinct chain once; per primitive [first count]
        chains    (vec (distinct (remove empty? (map :chain entries))))
        starts    (reductions + 0 (map count chains))
        chain-at  (zipmap chains starts)
        xforms    (vec (mapcat identity chains))
        mrows     (:rows @materials)
        trows     (:rows @textures)
        cam       (camera-row camera)]
    {:n-prims   (count prims)
     :prim-kind (int-array (map :kind prows))
     :prim-geom (double-array (mapcat :geom prows))
     :prim-mat  (int-array prim-mat)
     :n-mats    (count mrows)
     :mat-kind  (int-array (map :kind mrows))
     :mat-tex   (int-array (map :tex mrows))
     :mat-param (double-array (map :param mrows))
     :n-tex     (count trows)
     :tex-kind  (int-array (map :kind trows))
     :tex-param (double-array (mapcat :param trows))
     :tex-child (int-array (mapcat :child trows))
     :cam-kind  (int (:kind cam))
     :cam       (double-array (:cam cam))
     :prim-flip  (int-array (map :flip entries))
     :prim-xform (int-array (mapcat (fn [e] (if (empty? (:chain e)) [0 0] [(chain-at (:chain e)) (count (:chain e))])) entries))
     :n-xforms   (count xforms)
     :xform-kind  (int-array (map #(int (first %)) xforms))
     :xform-param (double-array (mapcat rest xforms))
     :media-calls (int-array media-calls)
     :media-narrow-from (int-array media-narrow-from)
     ;; 1 = RTMI_MEDIA_HITLIST: the world is a Hitlist, its narrowing reaches every medium; 2 = narrowed per call: Hitlists holding media below bvh-nodes
     :media-mode  (int (cond (= @media-modes #{:hitlist}) 1 (or (:narrowed @media-modes) (:hitlist @media-modes)) 2 :else 0))
     :uses-perlin (boolean (some #(#{3 4 5} (:kind %)) trows))
     :images      @images}))

;;; ---------------------------------------------------------------------------------------------
;;; render: replaces (dorun (cp/upmap ...)) of core.clj:100-108
;;; ---------------------------------------------------------------------------------------------

(defn- create-scene!
  "rtmi_scene_create_ex + everything a scene may need before its first render -- the namespace-level Perlin tables of the running
  JVM (perlin.clj:6-17), the decoded ImageMap pixels (texture.clj:126-133), the media call sequence -- on context `ctx` (a Pointer).
  Returns the scene Pointer.  Clones (rtmi_scene_clone) carry all of it."
  [ctx f]
  (let [scn (PointerByReference.)]
    (check (call-int "rtmi_scene_create_ex" ctx
                     (int (:n-prims f)) (:prim-kind f) (:prim-geom f) (:prim-mat f)
                     (int (:n-mats f)) (:mat-kind f) (:mat-tex f) (:mat-param f)
                     (int (:n-tex f)) (:tex-kind f) (:tex-param f) (:tex-child f)
                     (int (:cam-kind f)) (:cam f)
                     (:prim-flip f) (:prim-xform f) (int (:n-xforms f)) (:xform-kind f) (:xform-param f) scn))
    (let [scene (.getValue scn)]
      (when (:uses-perlin f)
        (let [vectors (double-array (mapcat v3 perlin/random-vectors))
              perm    (int-array (concat perlin/perm-x perlin/perm-y perlin/perm-z))]
          (check (call-int "rtmi_scene_set_perlin" scene vectors perm))))
      ;; ImageMap pixels: rows top-down, RGB (imagez get-pixel = BufferedImage.getRGB, texture.clj:76)
      (when (seq (:images f))
        (let [imgs (:images f)
              wh   (int-array (mapcat (fn [^java.awt.image.BufferedImage im] [(.getWidth im) (.getHeight im)]) imgs))
              px   (byte-array (mapcat (fn [^java.awt.image.BufferedImage im]
                                         (for [y (range (.getHeight im)) x (range (.getWidth im))
                                               :let [p (.getRGB im (int x) (int y))]
                                               sh [16 8 0]]
                                           (unchecked-byte (bit-and 0xff (bit-shift-right p sh)))))
                                       imgs))]
          (check (call-int "rtmi_scene_set_images" scene (int (count imgs)) wh px))))
      (if (= 2 (:media-mode f))
        (let [calls (:media-calls f)]
          (check (call-int "rtmi_scene_set_media_calls_narrowed" scene (int (alength ^ints calls)) calls (:media-narrow-from f))))
        (do
          (when (pos? (alength ^ints (:media-calls f)))
            (let [calls (:media-calls f)]
              (check (call-int "rtmi_scene_set_media_calls" scene (int (alength ^ints calls)) calls))))
          (when (pos? (:media-mode f))
            (check (call-int "rtmi_scene_set_media_mode" scene (int (:media-mode f)))))))
      scene)))

(defn render
  "Render scene {:camera :world} at nx x ny with ns samples per pixel on GPU `device`.
  Returns {:rgb8 byte-array (row 0 = top, RGB interleaved) :linear double-array
           :total-rays n :total-pixels n} (the counters of metrics.clj:8-9)."
  [scene nx ny ns & {:keys [depth seed device precision] :or {depth 50 seed 0x5eed0002 device 0 precision 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        npx  (* nx ny)
        lin  (double-array (* 3 npx))
        rgb  (byte-array (* 3 npx))
        cnt  (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render" scn (int nx) (int ny) (int ns) (int depth) (long seed) (int precision)
                           (int 0) (int 0) (int nx) (int ny) lin rgb cnt))
          {:rgb8 rgb :linear lin :total-rays (aget cnt 0) :total-pixels (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn set-camera
  "Give the live scene `scn` (the Pointer create-scene! returned) another camera record (PinholeCamera / ThinLensCamera) without a new
  scene: every render afterwards is, bit for bit, the render of a scene created with that camera.  Returns true when the library had to
  rebuild its trees (the scene holds MovingSpheres and the camera's shutter [t0, t1] lies outside the interval the scene was built for),
  false when only the camera changed.  A progressive frame started before the call is not continued (start a new one: s-first 0)."
  [scn camera]
  (let [row     (camera-row camera)
        cam     (double-array (:cam row))
        rebuilt (int-array 1)]
    (check (call-int "rtmi_scene_set_camera" scn (int (:kind row)) cam rebuilt))
    (= 1 (aget rebuilt 0))))

(defn render-views
  "Render scene {:camera :world} once per camera record of `cameras` -- a turntable, a fly-through, a shutter sweep -- from ONE device
  scene: the world is flattened, built and uploaded once, every view only moves the camera (set-camera).  Returns a vector of render's
  maps, one per camera, each equal to (render (assoc scene :camera c) ...)."
  [scene cameras nx ny ns & {:keys [depth seed device precision] :or {depth 50 seed 0x5eed0002 device 0 precision 0}}]
  (let [f   (flatten-scene scene)
        ctx (PointerByReference.)
        npx (* nx ny)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (mapv (fn [camera]
                  (let [lin (double-array (* 3 npx))
                        rgb (byte-array (* 3 npx))
                        cnt (long-array 2)]
                    (set-camera scn camera)
                    (check (call-int "rtmi_render" scn (int nx) (int ny) (int ns) (int depth) (long seed) (int precision)
                                     (int 0) (int 0) (int nx) (int ny) lin rgb cnt))
                    {:rgb8 rgb :linear lin :total-rays (aget cnt 0) :total-pixels (aget cnt 1)}))
                cameras)
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn set-materials
  "Give the live scene `scn` (the Pointer create-scene! returned for the flattened scene `flat`) other materials and textures without a
  new scene: `edited` is a scene {:camera :world} with the same primitives, or its flatten-scene map; its material and texture tables and
  its primitive-to-material assignment replace the scene's, the geometry and the camera stay.  Every render afterwards is, bit for bit, the
  render of a scene created from the edited arrays.  Returns true when the library had to rebuild the scene (the edit changes the number
  of materials or textures, or brings the first Perlin / ImageMap / Isotropic use into a scene of plain spheres -- the Perlin tables and
  images the scene already has stay), false when only the tables were rewritten where they lie.  A progressive frame started before the
  call is not continued (start a new one: s-first 0)."
  [scn flat edited]
  (let [e       (if (contains? edited :world) (flatten-scene edited) edited)
        rebuilt (int-array 1)]
    (when (not= (:n-prims e) (:n-prims flat))
      (throw (ex-info "set-materials: the edit has another primitive count" {:edit (:n-prims e) :scene (:n-prims flat)})))
    (check (call-int "rtmi_scene_set_materials" scn
                     (int (:n-mats e)) (:mat-kind e) (:mat-tex e) (:mat-param e)
                     (int (:n-tex e)) (:tex-kind e) (:tex-param e) (:tex-child e)
                     (:prim-mat e) rebuilt))
    (= 1 (aget rebuilt 0))))

(defn set-geometry
  "Move the primitives of the live scene `scn` (the Pointer create-scene! returned for the flattened scene `flat`) without a new scene:
  `edited` is a scene {:camera :world} with the same structure, or its flatten-scene map; its primitive geometry and the parameters of its
  Translate / RotateY records replace the scene's, the materials and the camera stay.  Every result afterwards is, bit for bit, that of a
  scene created from the edited arrays; the device refits the trees it has.  Counts, kinds, flips and the instance structure are not
  editable (ex-info).  :rebuild true asks for a fresh tree.  Returns {:rebuilt :displaced :nodes-refit :launches}: whether the library
  rebuilt the scene (the edit did not fit the built trees), how many primitives left their entry-grid cells and are now tested by every
  ray first (a rebuild brings them home), the node records refit and the launches that took.  A progressive frame started before the call
  is not continued (start a new one: s-first 0)."
  [scn flat edited & {:keys [rebuild] :or {rebuild false}}]
  (let [e    (if (contains? edited :world) (flatten-scene edited) edited)
        info (int-array 4)]
    (when (or (not= (:n-prims e) (:n-prims flat)) (not= (:n-xforms e) (:n-xforms flat)))
      (throw (ex-info "set-geometry: a changed count is a new scene" {:edit [(:n-prims e) (:n-xforms e)] :scene [(:n-prims flat) (:n-xforms flat)]})))
    (doseq [k [:prim-kind :prim-flip :prim-xform :xform-kind]]
      (when (not= (seq (k e)) (seq (k flat)))
        (throw (ex-info "set-geometry: kinds, flips and instance structure are not editable (a new scene)" {:array k}))))
    (check (call-int "rtmi_scene_set_geometry" scn
                     (int (:n-prims e)) (:prim-geom e) (int (:n-xforms e)) (:xform-param e)
                     (int (if rebuild 1 0)) info))
    {:rebuilt (= 1 (aget info 0)) :displaced (aget info 1) :nodes-refit (aget info 2) :launches (aget info 3)}))

(defn render-materials
  "Render scene {:camera :world} once per entry of `edits` -- scenes with the same primitives, or flatten-scene maps: a colour picker, a
  material library -- from ONE device scene: the world is flattened, built and uploaded once, every entry only rewrites the material
  tables (set-materials).  Returns a vector of render's maps plus :rebuilt, one per entry, each equal to (render entry ...)."
  [scene edits nx ny ns & {:keys [depth seed device precision] :or {depth 50 seed 0x5eed0002 device 0 precision 0}}]
  (let [f   (flatten-scene scene)
        ctx (PointerByReference.)
        npx (* nx ny)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (mapv (fn [edited]
                  (let [lin     (double-array (* 3 npx))
                        rgb     (byte-array (* 3 npx))
                        cnt     (long-array 2)
                        rebuilt (set-materials scn f edited)]
                    (check (call-int "rtmi_render" scn (int nx) (int ny) (int ns) (int depth) (long seed) (int precision)
                                     (int 0) (int 0) (int nx) (int ny) lin rgb cnt))
                    {:rgb8 rgb :linear lin :total-rays (aget cnt 0) :total-pixels (aget cnt 1) :rebuilt rebuilt}))
                edits)
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-progressive
  "Render scene {:camera :world} progressively on GPU `device` (rtmi_render_progressive): chunks of `chunk` samples up to ns, and after
  each chunk (on-chunk m) with m = what `render` returns for ns = k (bit for bit) plus :samples k and :stderr (double-array, per pixel the
  largest channel's standard error of the mean; ##Inf at k = 1).  The arrays are refilled by the next chunk: copy what must outlive it.
  on-chunk returning :stop ends the render early.  Returns the last m."
  [scene nx ny ns chunk on-chunk & {:keys [depth seed device precision] :or {depth 50 seed 0x5eed0002 device 0 precision 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        npx  (* nx ny)
        lin  (double-array (* 3 npx))
        rgb  (byte-array (* 3 npx))
        err  (double-array npx)
        cnt  (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (loop [k 0]
            (let [n (min chunk (- ns k))]
              (check (call-int "rtmi_render_progressive" scn (int nx) (int ny) (int k) (int n) (int depth) (long seed) (int precision)
                               (int 0) (int 0) (int nx) (int ny) lin rgb err cnt))
              (let [k' (+ k n)
                    m  {:samples k' :rgb8 rgb :linear lin :stderr err :total-rays (aget cnt 0) :total-pixels (aget cnt 1)}]
                (if (and (not= :stop (on-chunk m)) (< k' ns))
                  (recur k')
                  m))))
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-adaptive
  "Render scene {:camera :world} adaptively on GPU `device` (rtmi_render_adaptive): a first round of :first-round samples (default: chunk), then
  rounds of `chunk` samples up to ns per pixel.  After every round each 8x8 tile whose pixels all have a standard error <= eps stops taking
  samples; the render ends when no tile is active or at ns.  After each round (on-round m), m = {:samples k :rgb8 :linear :stderr
  :pixel-samples (int-array, the samples behind every pixel) :total-rays :total-pixels :active-tiles :total-tiles}; a pixel whose tile holds n
  samples equals `render` with ns = n there, bit for bit.  The arrays are refilled by the next round.  on-round returning :stop ends the
  render early.  Returns the last m."
  [scene nx ny ns chunk eps on-round & {:keys [first-round depth seed device precision] :or {depth 50 seed 0x5eed0002 device 0 precision 0}}]
  (let [f     (flatten-scene scene)
        ctx   (PointerByReference.)
        npx   (* nx ny)
        lin   (double-array (* 3 npx))
        rgb   (byte-array (* 3 npx))
        err   (double-array npx)
        smp   (int-array npx)
        cnt   (long-array 2)
        act   (int-array 1)
        tot   (int-array 1)
        pxs   (long-array 1)
        head  (or first-round chunk)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (loop [k 0]
            (let [n (min (if (zero? k) head chunk) (- ns k))]
              (check (call-int "rtmi_render_adaptive" scn (int nx) (int ny) (int k) (int n) (double eps) (int depth) (long seed) (int precision)
                               (int 0) (int 0) (int nx) (int ny) lin rgb err smp cnt))
              (check (call-int "rtmi_adaptive_status" (.getValue ctx) act tot pxs))
              (let [k' (+ k n)
                    m  {:samples k' :rgb8 rgb :linear lin :stderr err :pixel-samples smp :total-rays (aget cnt 0) :total-pixels (aget cnt 1)
                        :active-tiles (aget act 0) :total-tiles (aget tot 0)}]
                (if (and (not= :stop (on-round m)) (< k' ns) (pos? (aget act 0)))
                  (recur k')
                  m))))
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-features
  "First-hit feature buffers of scene {:camera :world} on GPU `device` (rtmi_render_features): per pixel the mean over the first segments of
  render samples 0 .. na-1 of albedo rgb, normal xyz, depth and coverage.  Returns {:features double-array [ny][nx][8] (row 0 = top)
  :feature-rays :total-pixels}.  seed must be the seed of the frame the features belong to."
  [scene nx ny na & {:keys [seed device precision] :or {seed 0x5eed0002 device 0 precision 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        ft   (double-array (* 8 nx ny))
        cnt  (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_features" scn (int nx) (int ny) (int na) (long seed) (int precision)
                           (int 0) (int 0) (int nx) (int ny) ft cnt))
          {:features ft :feature-rays (aget cnt 0) :total-pixels (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

;; the render stream's keys (rtmi_sample_key), restated: 64-bit wrapping arithmetic
(def ^:private stream-gold (unchecked-long 0x9E3779B97F4A7C15N))
(def ^:private stream-mul (unchecked-long 0xD6E8FEB86659FD93N))
(def ^:private stream-step (unchecked-long 0xD1B54A32D192ED03N))

(defn- mix64 [z]
  (let [z (bit-xor z (unsigned-bit-shift-right z 32))
        z (unchecked-multiply z stream-mul)
        z (bit-xor z (unsigned-bit-shift-right z 32))
        z (unchecked-multiply z stream-mul)]
    (bit-xor z (unsigned-bit-shift-right z 32))))

(defn sample-key
  "Stream key of (seed, pixel, sample) as a long: rtmi_sample_key."
  [seed pixel sample]
  (mix64 (unchecked-add (mix64 (bit-xor (unchecked-long seed) (unchecked-multiply stream-gold (unchecked-inc (long pixel)))))
                        (unchecked-multiply stream-step (unchecked-inc (long sample))))))

(defn render-rays
  "Paths from caller-supplied rays of scene {:camera :world} on GPU `device` (rtmi_render_rays): `rays` holds 7 doubles per ray (origin,
  direction, time), (* n-groups group) of them, ray r of group g at row (+ (* g group) r); the scene's camera is not read.  `keys` (longs, one
  per ray) key the rays' streams; without them ray r of group g is keyed (sample-key seed g (+ first-ray r)).  Every stream starts at draw
  `ctr0` (2 for a caller whose jitter took draws 0 and 1).  Returns {:mean double-array [n-groups][3], the group's rays folded in row order as a
  frame folds a pixel's samples, :stderr double-array [n-groups], :rays double-array [n][3], :state double-array [n-groups][10] (the groups'
  running records: pass it back as `state` with `first-ray` = the rays every group holds to continue them), :segments, :total-rays}."
  [scene rays n-groups group & {:keys [keys seed ctr0 depth device precision first-ray state]
                                :or {seed 0x5eed0002 ctr0 0 depth 50 device 0 precision 0 first-ray 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        n    (* n-groups group)
        rs   (double-array rays)
        ks   (long-array (or keys (for [g (range n-groups) r (range group)] (sample-key seed g (+ first-ray r)))))
        st   (double-array (or state (* 10 n-groups)))
        mean (double-array (* 3 n-groups))
        err  (double-array n-groups)
        out  (double-array (* 3 n))
        cnt  (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_rays" scn (int precision) (int n-groups) (int group) (int first-ray) rs ks (long seed) (int ctr0)
                           (int depth) st mean err out cnt))
          {:mean mean :stderr err :rays out :state st :segments (aget cnt 0) :total-rays (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-rays-nee
  "render-rays whose Lambertian vertices also sample the area lights (rtmi_render_rays_nee): one shadow ray per such vertex towards a point of one
  uniformly chosen light of `lights` (primitive indices out of scene-lights, at most 32; required here -- the C entry's NULL form, all eligible
  lights, is not bound; an empty list is render-rays).  The path itself is render-rays' bit for bit and the estimate has its expectation.  A scene
  that holds a ConstantMedium is refused.  Returns render-rays' map plus :shadow-rays and :shadow-rays-occluded."
  [scene rays n-groups group lights & {:keys [keys seed ctr0 depth device precision first-ray state]
                                       :or {seed 0x5eed0002 ctr0 0 depth 50 device 0 precision 0 first-ray 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        n    (* n-groups group)
        rs   (double-array rays)
        ks   (long-array (or keys (for [g (range n-groups) r (range group)] (sample-key seed g (+ first-ray r)))))
        lp   (int-array (if (seq lights) lights [0]))
        nl   (count lights)
        st   (double-array (or state (* 10 n-groups)))
        mean (double-array (* 3 n-groups))
        err  (double-array n-groups)
        out  (double-array (* 3 n))
        cnt  (long-array 4)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_rays_nee" scn (int precision) (int n-groups) (int group) (int first-ray) rs ks (long seed) (int ctr0)
                           (int depth) (int nl) lp st mean err out cnt))
          {:mean mean :stderr err :rays out :state st :segments (aget cnt 0) :total-rays (aget cnt 1)
           :shadow-rays (aget cnt 2) :shadow-rays-occluded (aget cnt 3)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-rays-mis
  "render-rays-nee under multiple importance sampling (rtmi_render_rays_mis): the same paths and shadow rays, but the light sample and the path's own
  scatter share each lamp's emission by the balance heuristic, so no contribution exceeds attenuation x emission -- no bright outliers beside a lamp.
  `light-choice` 0 picks the light uniformly, 1 in proportion to its power.  `lights` as for render-rays-nee (required; an empty list is render-rays).
  Returns render-rays-nee's map."
  [scene rays n-groups group lights & {:keys [keys seed ctr0 depth device precision first-ray state light-choice]
                                       :or {seed 0x5eed0002 ctr0 0 depth 50 device 0 precision 0 first-ray 0 light-choice 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        n    (* n-groups group)
        rs   (double-array rays)
        ks   (long-array (or keys (for [g (range n-groups) r (range group)] (sample-key seed g (+ first-ray r)))))
        lp   (int-array (if (seq lights) lights [0]))
        nl   (count lights)
        st   (double-array (or state (* 10 n-groups)))
        mean (double-array (* 3 n-groups))
        err  (double-array n-groups)
        out  (double-array (* 3 n))
        cnt  (long-array 4)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_rays_mis" scn (int precision) (int n-groups) (int group) (int first-ray) rs ks (long seed) (int ctr0)
                           (int depth) (int nl) lp (int light-choice) st mean err out cnt))
          {:mean mean :stderr err :rays out :state st :segments (aget cnt 0) :total-rays (aget cnt 1)
           :shadow-rays (aget cnt 2) :shadow-rays-occluded (aget cnt 3)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-rays-ris
  "render-rays-mis whose light is chosen by looking at the vertex (rtmi_render_rays_ris, THE PROPOSAL RULE of rtmi.h): every listed light (at most
  32) proposes one point at each Lambertian vertex, each proposal is weighed by what it would contribute if it were visible, and a one-pass weighted
  reservoir keeps the one the shadow ray is sent to.  The path and the closing emission are render-rays-mis'; there is no light choice.  `lights` as
  for render-rays-nee (required; an empty list is render-rays).  Returns render-rays-nee's map."
  [scene rays n-groups group lights & {:keys [keys seed ctr0 depth device precision first-ray state]
                                       :or {seed 0x5eed0002 ctr0 0 depth 50 device 0 precision 0 first-ray 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        n    (* n-groups group)
        rs   (double-array rays)
        ks   (long-array (or keys (for [g (range n-groups) r (range group)] (sample-key seed g (+ first-ray r)))))
        lp   (int-array (if (seq lights) lights [0]))
        nl   (count lights)
        st   (double-array (or state (* 10 n-groups)))
        mean (double-array (* 3 n-groups))
        err  (double-array n-groups)
        out  (double-array (* 3 n))
        cnt  (long-array 4)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_rays_ris" scn (int precision) (int n-groups) (int group) (int first-ray) rs ks (long seed) (int ctr0)
                           (int depth) (int nl) lp st mean err out cnt))
          {:mean mean :stderr err :rays out :state st :segments (aget cnt 0) :total-rays (aget cnt 1)
           :shadow-rays (aget cnt 2) :shadow-rays-occluded (aget cnt 3)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-lit
  "A light-sampled nx x ny frame of scene {:camera :world} from its own camera, the camera rays built on the device (rtmi_render_lit): samples
  [s-first, s-first + ns) of every pixel -- the keys, film jitter, lens draws and streams of `render` -- under `estimator` 0 (the plain path:
  `render`'s frame bit for bit), 1 (the NEE rule) or 2 (the MIS rule, with `light-choice` 0 uniform / 1 by power).  `lights` as for render-rays-nee
  (required; estimator 0 does not read them, an empty list is the plain path).  Returns {:linear double-array [ny * nx][3] (row 0 = top), :rgb8
  byte-array, :stderr double-array [ny * nx], :rays double-array [nx * ny * ns][3] (sample s of pixel g at row (+ (* g ns) s)), :camera
  double-array [nx * ny * ns][8] (origin, direction, time, the stream position behind the camera), :state double-array [nx * ny][10] (pass it back
  as `state` with `s-first` = the samples every pixel holds to refine the frame), :segments, :total-rays, :shadow-rays, :shadow-rays-occluded}."
  [scene nx ny ns lights & {:keys [estimator light-choice seed depth device precision s-first state]
                            :or {estimator 2 light-choice 0 seed 0x5eed0002 depth 50 device 0 precision 0 s-first 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        npx  (* nx ny)
        n    (* npx ns)
        lp   (int-array (if (seq lights) lights [0]))
        nl   (count lights)
        st   (double-array (or state (* 10 npx)))
        lin  (double-array (* 3 npx))
        rgb8 (byte-array (* 3 npx))
        err  (double-array npx)
        out  (double-array (* 3 n))
        cam  (double-array (* 8 n))
        cnt  (long-array 4)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_lit" scn (int precision) (int nx) (int ny) (int s-first) (int ns) (int depth) (long seed) (int estimator)
                           (int nl) lp (int light-choice) st lin rgb8 err out cam cnt))
          {:linear lin :rgb8 rgb8 :stderr err :rays out :camera cam :state st :segments (aget cnt 0) :total-rays (aget cnt 1)
           :shadow-rays (aget cnt 2) :shadow-rays-occluded (aget cnt 3)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-rays-vol
  "render-rays-nee / render-rays-mis on a scene that holds a ConstantMedium (rtmi_render_rays_vol): the vertices inside a medium sample the lights
  too, with the uniform sphere's density, and every shadow ray draws its own free-flight distances from the media it crosses, so the unoccluded flag
  estimates the transmittance.  `estimator` 1 is the NEE rule, 2 the MIS rule (with `light-choice` 0 uniform / 1 by power).  `lights` as for
  render-rays-nee (required; an empty list is render-rays).  On a scene without media the result is the sibling's bit for bit.  Returns
  render-rays-nee's map."
  [scene rays n-groups group lights & {:keys [keys seed ctr0 depth device precision first-ray state estimator light-choice]
                                       :or {seed 0x5eed0002 ctr0 0 depth 50 device 0 precision 0 first-ray 0 estimator 2 light-choice 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        n    (* n-groups group)
        rs   (double-array rays)
        ks   (long-array (or keys (for [g (range n-groups) r (range group)] (sample-key seed g (+ first-ray r)))))
        lp   (int-array (if (seq lights) lights [0]))
        nl   (count lights)
        st   (double-array (or state (* 10 n-groups)))
        mean (double-array (* 3 n-groups))
        err  (double-array n-groups)
        out  (double-array (* 3 n))
        cnt  (long-array 4)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_rays_vol" scn (int precision) (int n-groups) (int group) (int first-ray) rs ks (long seed) (int ctr0)
                           (int depth) (int estimator) (int nl) lp (int light-choice) st mean err out cnt))
          {:mean mean :stderr err :rays out :state st :segments (aget cnt 0) :total-rays (aget cnt 1)
           :shadow-rays (aget cnt 2) :shadow-rays-occluded (aget cnt 3)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-lit-vol
  "render-lit on a scene that holds a ConstantMedium (rtmi_render_lit_vol): the same frame rule, state and outputs under the volume rule, `estimator`
  1 (the NEE rule) or 2 (the MIS rule) only.  make-final, the smoke Cornell box and make-subsurface-sphere render through it.  Returns render-lit's map."
  [scene nx ny ns lights & {:keys [estimator light-choice seed depth device precision s-first state]
                            :or {estimator 2 light-choice 0 seed 0x5eed0002 depth 50 device 0 precision 0 s-first 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        npx  (* nx ny)
        n    (* npx ns)
        lp   (int-array (if (seq lights) lights [0]))
        nl   (count lights)
        st   (double-array (or state (* 10 npx)))
        lin  (double-array (* 3 npx))
        rgb8 (byte-array (* 3 npx))
        err  (double-array npx)
        out  (double-array (* 3 n))
        cam  (double-array (* 8 n))
        cnt  (long-array 4)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_lit_vol" scn (int precision) (int nx) (int ny) (int s-first) (int ns) (int depth) (long seed) (int estimator)
                           (int nl) lp (int light-choice) st lin rgb8 err out cam cnt))
          {:linear lin :rgb8 rgb8 :stderr err :rays out :camera cam :state st :segments (aget cnt 0) :total-rays (aget cnt 1)
           :shadow-rays (aget cnt 2) :shadow-rays-occluded (aget cnt 3)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn query-hits
  "The closest hit of every caller-supplied ray of scene {:camera :world} on GPU `device` (rtmi_query_hits): `rays` holds 7 doubles per ray
  (origin, direction, time), `n` of them; the scene's camera is not read.  Every ray takes (t-min, t-max), or its own pair of `t-range`
  (2 doubles per ray).  `keys` (longs, one per ray) key the streams a ConstantMedium draws from, each starting at draw `ctr0`; without them every
  ray is keyed 0.  Returns {:hits double-array [n][12] = hit?, prim, t, p xyz, normal xyz, u, v, material (zeros on a miss), :rays n,
  :rays-hit}."
  [scene rays n & {:keys [keys t-range t-min t-max ctr0 device precision]
                   :or {t-min 0.001 t-max 3.4028234663852886e38 ctr0 0 device 0 precision 0}}]
  (let [f   (flatten-scene scene)
        ctx (PointerByReference.)
        rs  (double-array rays)
        tr  (double-array (or t-range (mapcat (fn [_] [t-min t-max]) (range n))))
        ks  (long-array (or keys n))
        out (double-array (* 12 n))
        cnt (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_query_hits" scn (int precision) (int n) rs tr (double t-min) (double t-max) ks (int (if keys ctr0 0)) out cnt))
          {:hits out :rays (aget cnt 0) :rays-hit (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn occluded
  "Is anything hit within each ray's range (rtmi_query_occluded)?  (* n-groups group) rays as for query-hits, ray r of group g at row
  (+ (* g group) r).  The search leaves at the first primitive that accepts the ray.  Returns {:occluded byte-array [n], 1 where query-hits
  would report a hit, :count int-array [n-groups] = occluded rays per group, :rays n, :rays-occluded}."
  [scene rays n-groups group & {:keys [keys t-range t-min t-max ctr0 device precision]
                                :or {t-min 0.001 t-max 3.4028234663852886e38 ctr0 0 device 0 precision 0}}]
  (let [f     (flatten-scene scene)
        ctx   (PointerByReference.)
        n     (* n-groups group)
        rs    (double-array rays)
        tr    (double-array (or t-range (mapcat (fn [_] [t-min t-max]) (range n))))
        ks    (long-array (or keys n))
        flags (byte-array n)
        per   (int-array n-groups)
        cnt   (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_query_occluded" scn (int precision) (int n-groups) (int group) rs tr (double t-min) (double t-max) ks
                           (int (if keys ctr0 0)) flags per cnt))
          {:occluded flags :count per :rays (aget cnt 0) :rays-occluded (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn occlusion-hemisphere
  "n-dirs cosine-weighted occlusion rays from each of n-points hit records, generated on the device (rtmi_occlusion_hemisphere): `hits` holds
  12 doubles per point as query-hits returns them, `view` the 7 doubles of the ray that found each point (its direction picks the side of the
  surface, its time is the new rays'); `view` is required here (7 * n-points doubles -- the C entry's NULL form is not bound).  Direction k of point g draws from the stream keyed (sample-key seed g (+ first k)).  Returns
  {:occluded byte-array [n], :count int-array [n-points], :out-rays double-array [n][7] (zeros where a point yields no ray), :rays, :rays-occluded}."
  [scene hits view n-points n-dirs & {:keys [first seed t-min t-max device precision]
                                      :or {first 0 seed 0x5EED0002 t-min 0.001 t-max 3.4028234663852886e38 device 0 precision 0}}]
  (let [f     (flatten-scene scene)
        ctx   (PointerByReference.)
        n     (* n-points n-dirs)
        hs    (double-array hits)
        vw    (double-array view)
        flags (byte-array n)
        per   (int-array n-points)
        out   (double-array (* 7 n))
        cnt   (long-array 2)]
    (when-not (and (= (alength hs) (* 12 n-points)) (= (alength vw) (* 7 n-points)))
      (throw (IllegalArgumentException. "hits must hold 12 and view 7 doubles per point")))
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_occlusion_hemisphere" scn (int precision) (int n-points) hs vw (int n-dirs) (int first) (long seed) (double 0.0)
                           (double t-min) (double t-max) flags per out cnt))
          {:occluded flags :count per :out-rays out :rays (aget cnt 0) :rays-occluded (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn occlusion-targets
  "One occlusion ray from each of n-points hit records towards each of n-targets points, generated on the device (rtmi_occlusion_targets):
  `targets` holds 3 doubles per target, `hits` and `view` as for occlusion-hemisphere (of `view` only the time is read; required as there).  The direction is
  target - point, so (t-min, t-max) = (0.001, 0.999) asks \"up to the light\".  Returns what occlusion-hemisphere returns, one group per point."
  [scene hits view n-points targets n-targets & {:keys [t-min t-max device precision] :or {t-min 0.001 t-max 0.999 device 0 precision 0}}]
  (let [f     (flatten-scene scene)
        ctx   (PointerByReference.)
        n     (* n-points n-targets)
        hs    (double-array hits)
        vw    (double-array view)
        tg    (double-array targets)
        flags (byte-array n)
        per   (int-array n-points)
        out   (double-array (* 7 n))
        cnt   (long-array 2)]
    (when-not (and (= (alength hs) (* 12 n-points)) (= (alength vw) (* 7 n-points)) (= (alength tg) (* 3 n-targets)))
      (throw (IllegalArgumentException. "hits must hold 12 and view 7 doubles per point, targets 3 per target")))
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_occlusion_targets" scn (int precision) (int n-points) hs vw (int n-targets) tg (double 0.0) (double t-min)
                           (double t-max) flags per out cnt))
          {:occluded flags :count per :out-rays out :rays (aget cnt 0) :rays-occluded (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn ambient-occlusion
  "Ambient occlusion of the nx x ny view of scene {:camera :world}, the whole pass on the device (rtmi_ambient_occlusion): the first hits of the
  pixel-centre rays, n-dirs cosine-weighted rays per hit on the viewer's side with t-range (0.001, radius), visibility = 1 - occluded / n-dirs
  and 1 where the primary ray missed.  Returns {:visibility double-array [ny * nx] (row 0 = top), :count int-array, :hits double-array
  [ny * nx][12], :rays, :rays-occluded}; `first` offsets the directions, so a caller accumulates :count over calls."
  [scene nx ny n-dirs radius & {:keys [first seed device precision] :or {first 0 seed 0x5EED0002 device 0 precision 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        n    (* nx ny)
        vis  (double-array n)
        per  (int-array n)
        hits (double-array (* 12 n))
        cnt  (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_ambient_occlusion" scn (int precision) (int nx) (int ny) (int n-dirs) (int first) (double radius) (long seed)
                           vis per hits cnt))
          {:visibility vis :count per :hits hits :rays (aget cnt 0) :rays-occluded (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn scene-lights
  "The primitives of scene {:camera :world} a light sample can be placed on (rtmi_scene_lights), in primitive order, as a vector of indices
  into the flattened primitive list: spheres and axis-aligned rectangles without a Translate / RotateY chain whose material is a DiffuseLight
  over a Constant texture.  Moving, triangle, instanced, gradient and image emitters are left out; that is no error."
  [scene & {:keys [device] :or {device 0}}]
  (let [f     (flatten-scene scene)
        ctx   (PointerByReference.)
        prims (int-array 32)
        cnt   (int-array 1)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_scene_lights" scn (int 32) prims cnt))
          (vec (take (min 32 (aget cnt 0)) prims))
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn direct-irradiance
  "The direct irradiance at each of n-points hit records (rtmi_direct_irradiance): n-samples points on each of the lights `lights` (primitive
  indices out of scene-lights, at most 32; required here -- the C entry's NULL form, all eligible lights, is not bound), one shadow ray each,
  weighted by both cosines, the inverse square and the light's area.  `hits` holds 12 doubles per point as query-hits returns them, `view` the
  7 doubles of the ray that found each point (required, as for occlusion-hemisphere).  Item (g * n-samples + k) * n-lights + l draws from the
  stream keyed (sample-key seed (+ (* g n-lights) l) (+ first k)).  Returns {:irradiance double-array [n-points][3], :contrib double-array
  [items][3], :occluded byte-array [items], :out-rays double-array [items][7], :rays, :rays-occluded}."
  [scene hits view n-points lights n-samples & {:keys [first seed lambert-only device precision]
                                                 :or {first 0 seed 0x5EED0002 lambert-only false device 0 precision 0}}]
  (let [f       (flatten-scene scene)
        ctx     (PointerByReference.)
        lp      (int-array lights)
        nl      (alength lp)
        n       (* n-points n-samples nl)
        hs      (double-array hits)
        vw      (double-array view)
        state   (double-array (* 4 n-points))
        irr     (double-array (* 3 n-points))
        contrib (double-array (* 3 n))
        flags   (byte-array n)
        out     (double-array (* 7 n))
        cnt     (long-array 2)]
    (when-not (and (= (alength hs) (* 12 n-points)) (= (alength vw) (* 7 n-points)))
      (throw (IllegalArgumentException. "hits must hold 12 and view 7 doubles per point")))
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_direct_irradiance" scn (int precision) (int n-points) hs vw (int nl) lp (int n-samples) (int first) (long seed)
                           (double 0.0) (int (if lambert-only 1 0)) state irr contrib flags out cnt))
          {:irradiance irr :contrib contrib :occluded flags :out-rays out :rays (aget cnt 0) :rays-occluded (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-direct
  "The nx x ny view of scene {:camera :world} lit directly, the whole pass on the device (rtmi_render_direct): the first hits of the
  pixel-centre rays, n-samples shadow rays per hit towards every light of scene-lights, then per pixel: an emitter shows its emission, a
  Lambertian surface albedo * E / pi, anything else and a miss is black.  Returns {:linear double-array [ny * nx][3] (row 0 = top), :rgb8
  byte-array, :hits double-array [ny * nx][12], :rays, :rays-occluded}."
  [scene nx ny n-samples & {:keys [seed device precision] :or {seed 0x5EED0002 device 0 precision 0}}]
  (let [f     (flatten-scene scene)
        ctx   (PointerByReference.)
        n     (* nx ny)
        state (double-array (* 4 n))
        lin   (double-array (* 3 n))
        rgb8  (byte-array (* 3 n))
        hits  (double-array (* 12 n))
        cnt   (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_direct" scn (int precision) (int nx) (int ny) (int n-samples) (int 0) (long seed) state lin rgb8 hits cnt))
          {:linear lin :rgb8 rgb8 :hits hits :rays (aget cnt 0) :rays-occluded (aget cnt 1)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn pick
  "What lies under pixel (column i, row j from the top) of an nx x ny view of scene {:camera :world}: nil, or {:prim :material :t :p :normal
  :uv} of the closest hit of the ray from the camera's origin (a thin lens: its lens centre) through the pixel's centre -- u = (i + 1/2) / nx,
  v = (ny - 1 - j + 1/2) / ny, direction lleft + u horiz + v vert - origin in get-ray's operation order."
  [scene nx ny i j & {:keys [device] :or {device 0}}]
  (let [cam (vec (:cam (camera-row (:camera scene))))
        u   (/ (+ (double i) 0.5) (double nx))
        v   (/ (+ (- (double (dec ny)) (double j)) 0.5) (double ny))
        dir (fn [k] (+ (+ (+ (cam (+ 3 k)) (* (cam (+ 6 k)) u)) (* (cam (+ 9 k)) v)) (- (cam k))))
        ray [(cam 0) (cam 1) (cam 2) (dir 0) (dir 1) (dir 2) (if (= 0 (:kind (camera-row (:camera scene)))) 0.0 (cam 22))]
        h   (vec (:hits (query-hits scene ray 1 :device device)))]
    (when-not (zero? (h 0))
      {:prim (long (h 1)) :material (long (h 11)) :t (h 2) :p (subvec h 3 6) :normal (subvec h 6 9) :uv (subvec h 9 11)})))

(defn denoise
  "Edge-aware a-trous filter (rtmi_denoise) of a frame: linear [ny][nx][3] (:linear of render / render-adaptive), stderr [ny][nx] (:stderr)
  and features [ny][nx][8] (:features of render-features), `iterations` passes (0 .. 8).  A sigma of 0 switches its term off.  Returns
  {:linear :rgb8 :stderr} of the filtered frame.  (A frame without a noise estimate or without features: pass NULL for it to rtmi_denoise.)"
  [nx ny linear stderr features & {:keys [iterations sigma-c sigma-n sigma-a sigma-d device]
                                   :or {iterations 5 sigma-c 4.0 sigma-n 0.5 sigma-a 0.2 sigma-d 0.2 device 0}}]
  (let [ctx  (PointerByReference.)
        npx  (* nx ny)
        lin  (double-array linear)
        se   (double-array stderr)
        ft   (double-array features)
        out  (double-array (* 3 npx))
        rgb  (byte-array (* 3 npx))
        err  (double-array npx)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (check (call-int "rtmi_denoise" (.getValue ctx) (int nx) (int ny) lin se ft (int iterations) (double sigma-c) (double sigma-n)
                       (double sigma-a) (double sigma-d) out rgb err))
      {:linear out :rgb8 rgb :stderr err}
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn reproject
  "Temporal accumulation (rtmi_reproject): blend the previous view's result into the current frame where both see the same surface.
  `prev` = {:cam-kind :cam :linear :weight :stderr :features} -- the camera the history was seen with (:cam-kind / :cam of flatten-scene),
  its colour [ny][nx][3], the samples accumulated behind every pixel [ny][nx] (doubles), its standard error [ny][nx] and the previous view's
  features [ny][nx][8]; `cur` = {:cam-kind :cam :linear :stderr :features} of the current frame, `cur-weight` its samples per pixel.
  :max-history caps the weight a history may count for (Double/POSITIVE_INFINITY = no cap); a sigma of 0 switches its test off.
  Returns {:linear :rgb8 :weight :stderr :counters [pixels, pixels that took history]}: feed :linear, :weight and :stderr back as the next
  call's `prev`, with the current features and camera.  (A frame without a noise estimate: pass NULL for both stderr planes and for
  out_stderr to rtmi_reproject.)"
  [nx ny prev cur cur-weight & {:keys [max-history sigma-d sigma-n sigma-a device]
                                :or {max-history 8.0 sigma-d 0.1 sigma-n 0.0 sigma-a 0.0 device 0}}]
  (let [ctx  (PointerByReference.)
        npx  (* nx ny)
        pcam (double-array (:cam prev))
        ccam (double-array (:cam cur))
        plin (double-array (:linear prev))
        pw   (double-array (:weight prev))
        pse  (double-array (:stderr prev))
        pft  (double-array (:features prev))
        clin (double-array (:linear cur))
        cse  (double-array (:stderr cur))
        cft  (double-array (:features cur))
        out  (double-array (* 3 npx))
        rgb  (byte-array (* 3 npx))
        wgt  (double-array npx)
        err  (double-array npx)
        cnt  (long-array 2)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (check (call-int "rtmi_reproject" (.getValue ctx) (int nx) (int ny) (int (:cam-kind prev)) pcam (int (:cam-kind cur)) ccam
                       plin pw pse pft clin cse cft (double cur-weight) (double max-history) (double sigma-d) (double sigma-n)
                       (double sigma-a) out rgb wgt err cnt))
      {:linear out :rgb8 rgb :weight wgt :stderr err :counters (vec cnt)}
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn adaptive-retire
  "Retire the active tiles of context `ctx`'s progressive frame whose pixels all pass noise <= eps (rtmi_adaptive_retire; a NaN fails): `noise`
  holds [ny][nx] doubles of the whole frame, row 0 = top -- :stderr of `denoise` as it is.  Adds no samples.  Returns the number of tiles this
  call retired.  The device form (rtmi_adaptive_retire_device) takes an HBM pointer and a stream instead: see adaptive-retire-device."
  [ctx nx ny noise eps]
  (let [m   (double-array noise)
        out (int-array 1)]
    (check (call-int "rtmi_adaptive_retire" ctx (int nx) (int ny) m (double eps) out))
    (aget out 0)))

(defn adaptive-retire-device
  "adaptive-retire on a map resident in HBM: `d-noise` and `stream` are com.sun.jna.Pointer (stream nil = the context's own stream).  The call
  synchronises the stream once, at its end.  (The one device-buffer entry this file binds: the conformance reader has no category for device
  pointers, so the call is made on the Function itself, with the same coercions as every call-int form.)"
  [ctx nx ny ^Pointer d-noise eps ^Pointer stream]
  (let [out (int-array 1)]
    (check (.invokeInt (cfn "rtmi_adaptive_retire_device") (object-array [ctx (int nx) (int ny) d-noise (double eps) out stream])))
    (aget out 0)))

(defn tiles-retire
  "The stateless adaptive-retire (rtmi_tiles_retire): of the 8x8 tiles listed in `tiles` (global indices, row-major over the frame's tiles) those
  with a pixel inside the image that fails noise <= eps (NaN and +inf fail), in the list's order, as a vector.  `noise` holds [ny][nx] doubles of the
  whole frame, row 0 = top -- :stderr of render-lit-tiles or of `denoise` as it is.  No frame of context `ctx` is read or changed."
  [ctx nx ny noise eps tiles]
  (let [m   (double-array noise)
        tin (int-array tiles)
        out (int-array (max 1 (count tiles)))
        n   (int-array 1)]
    (check (call-int "rtmi_tiles_retire" ctx (int nx) (int ny) m (double eps) (int (count tiles)) tin out n))
    (vec (take (aget n 0) out))))

(defn render-lit-tiles
  "render-lit / render-lit-vol over a list of 8x8 tiles (rtmi_render_lit_tiles): samples [s-first, s-first + ns) of the pixels of the tiles in
  `tiles` (strictly ascending global tile indices, rtmi_adaptive_active_tiles' numbering) and of no other pixel.  `frame` = {:linear :rgb8 :stderr
  :state} holds the whole frame's arrays (double-array [ny * nx][3], byte-array [ny * nx][3], double-array [ny * nx], double-array [nx * ny][10]) and
  is written IN PLACE: the listed pixels take the fold's values, every other element keeps what it held; nil starts a frame of zeros.  :volume true
  runs the volume rule (estimator 1 or 2).  Returns {:linear :rgb8 :stderr :state (the frame's arrays), :rays double-array [n-tiles * 64 * ns][3] and
  :camera double-array [...][8] in THE TILE ORDER of rtmi.h (sample s of local pixel l of entry k at row (+ (* (+ (* k 64) l) ns) s); zeros where the
  pixel lies outside the image), :segments, :total-rays, :shadow-rays, :shadow-rays-occluded} of this call alone."
  [scene nx ny ns lights tiles frame & {:keys [estimator light-choice volume seed depth device precision s-first]
                                        :or {estimator 2 light-choice 0 volume false seed 0x5eed0002 depth 50 device 0 precision 0 s-first 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        npx  (* nx ny)
        nt   (count tiles)
        n    (* nt 64 ns)
        lp   (int-array (if (seq lights) lights [0]))
        nl   (count lights)
        tl   (int-array (if (seq tiles) tiles [0]))
        st   (double-array (or (:state frame) (* 10 npx)))
        lin  (double-array (or (:linear frame) (* 3 npx)))
        rgb8 (byte-array (or (:rgb8 frame) (* 3 npx)))
        err  (double-array (or (:stderr frame) npx))
        out  (double-array (max 1 (* 3 n)))
        cam  (double-array (max 1 (* 8 n)))
        cnt  (long-array 4)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_lit_tiles" scn (int precision) (int nx) (int ny) (int s-first) (int ns) (int depth) (long seed) (int estimator)
                           (int nl) lp (int light-choice) (int (if volume 1 0)) (int nt) tl st lin rgb8 err out cam cnt))
          {:linear lin :rgb8 rgb8 :stderr err :state st :rays out :camera cam :segments (aget cnt 0) :total-rays (aget cnt 1)
           :shadow-rays (aget cnt 2) :shadow-rays-occluded (aget cnt 3)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-lit-ris
  "render-lit-tiles under THE PROPOSAL RULE of rtmi.h (rtmi_render_lit_ris): the frame of the scene's own camera whose every light proposes a point
  at each Lambertian vertex, one shadow ray sent to the candidate a weighted reservoir keeps.  `tiles`: strictly ascending global tile indices, or
  nil for every tile of the frame in ascending order, which reproduces every output of the whole-frame call.  `frame`, the in-place arrays and the
  returned map are render-lit-tiles'; there is no estimator, light choice or volume form."
  [scene nx ny ns lights tiles frame & {:keys [seed depth device precision s-first]
                                        :or {seed 0x5eed0002 depth 50 device 0 precision 0 s-first 0}}]
  (let [f    (flatten-scene scene)
        ctx  (PointerByReference.)
        npx  (* nx ny)
        tiles (or tiles (range (* (quot (+ nx 7) 8) (quot (+ ny 7) 8))))
        nt   (count tiles)
        n    (* nt 64 ns)
        lp   (int-array (if (seq lights) lights [0]))
        nl   (count lights)
        tl   (int-array (if (seq tiles) tiles [0]))
        st   (double-array (or (:state frame) (* 10 npx)))
        lin  (double-array (or (:linear frame) (* 3 npx)))
        rgb8 (byte-array (or (:rgb8 frame) (* 3 npx)))
        err  (double-array (or (:stderr frame) npx))
        out  (double-array (max 1 (* 3 n)))
        cam  (double-array (max 1 (* 8 n)))
        cnt  (long-array 4)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_lit_ris" scn (int precision) (int nx) (int ny) (int s-first) (int ns) (int depth) (long seed)
                           (int nl) lp (int nt) tl st lin rgb8 err out cam cnt))
          {:linear lin :rgb8 rgb8 :stderr err :state st :rays out :camera cam :segments (aget cnt 0) :total-rays (aget cnt 1)
           :shadow-rays (aget cnt 2) :shadow-rays-occluded (aget cnt 3)}
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-lit-adaptive
  "A light-sampled frame of scene {:camera :world} refined adaptively on GPU `device`: every 8x8 tile listed, then rounds of rtmi_render_lit_tiles
  (`first-round` samples, default `chunk`, then `chunk`), each followed by rtmi_tiles_retire of the tiles whose standard error is <= eps everywhere,
  until no tile is listed or `ns` is reached.  The list is compacted in place.  After each round (on-round m), m = {:samples k :linear :rgb8 :stderr
  :state :rays :camera (the round's rows in THE TILE ORDER; all refilled by the next round) :active-tiles :total-tiles :segments :total-rays :shadow-rays :shadow-rays-occluded (summed over the rounds)};
  on-round returning :stop ends the render early.  A pixel whose tile took n samples equals render-lit with ns = n there bit for bit; the samples a
  pixel holds are slot 9 of its :state record.  Returns the last m."
  [scene nx ny ns chunk eps lights on-round & {:keys [first-round estimator light-choice volume seed depth device precision]
                                               :or {estimator 2 light-choice 0 volume false seed 0x5eed0002 depth 50 device 0 precision 0}}]
  (let [f     (flatten-scene scene)
        ctx   (PointerByReference.)
        npx   (* nx ny)
        total (* (quot (+ nx 7) 8) (quot (+ ny 7) 8))
        lp    (int-array (if (seq lights) lights [0]))
        nl    (count lights)
        tl    (int-array (range total))
        st    (double-array (* 10 npx))
        lin   (double-array (* 3 npx))
        rgb8  (byte-array (* 3 npx))
        err   (double-array npx)
        cnt   (long-array 4)
        sums  (long-array 4)
        left  (int-array 1)
        head  (or first-round chunk)
        rows  (* total 64 (max head chunk))
        out   (double-array (* 3 rows))
        cam   (double-array (* 8 rows))]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (loop [k 0 nt total]
            (let [n (min (if (zero? k) head chunk) (- ns k))]
              (check (call-int "rtmi_render_lit_tiles" scn (int precision) (int nx) (int ny) (int k) (int n) (int depth) (long seed) (int estimator)
                               (int nl) lp (int light-choice) (int (if volume 1 0)) (int nt) tl st lin rgb8 err out cam cnt))
              (check (call-int "rtmi_tiles_retire" (.getValue ctx) (int nx) (int ny) err (double eps) (int nt) tl tl left))
              (dotimes [i 4] (aset sums i (+ (aget sums i) (aget cnt i))))
              (let [k' (+ k n)
                    m  {:samples k' :linear lin :rgb8 rgb8 :stderr err :state st :rays out :camera cam :active-tiles (aget left 0) :total-tiles total
                        :segments (aget sums 0) :total-rays (aget sums 1) :shadow-rays (aget sums 2) :shadow-rays-occluded (aget sums 3)}]
                (if (and (not= :stop (on-round m)) (< k' ns) (pos? (aget left 0)))
                  (recur k' (aget left 0))
                  m))))
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-adaptive-denoised
  "Render scene {:camera :world} adaptively on GPU `device` for a frame that is denoised anyway: the feature buffers once (:feature-samples,
  default 4), then rounds as in render-adaptive; per round rtmi_render_adaptive with the raw rule at eps 0 (only tiles whose samples are all
  equal retire), rtmi_denoise of the frame with its standard error and the features (:iterations, :sigma-c ... as `denoise`), and
  rtmi_adaptive_retire of the tiles whose FILTERED standard error is <= eps everywhere.  After each round (on-round m), m = what render-adaptive
  passes (with :active-tiles taken after the retirement) plus :denoised {:linear :rgb8 :stderr}.  The arrays are refilled by the next round.
  on-round returning :stop ends the render early.  Returns the last m."
  [scene nx ny ns chunk eps on-round & {:keys [first-round feature-samples iterations sigma-c sigma-n sigma-a sigma-d depth seed device precision]
                                        :or {feature-samples 4 iterations 5 sigma-c 4.0 sigma-n 0.5 sigma-a 0.2 sigma-d 0.2
                                             depth 50 seed 0x5eed0002 device 0 precision 0}}]
  (let [f     (flatten-scene scene)
        ctx   (PointerByReference.)
        npx   (* nx ny)
        lin   (double-array (* 3 npx))
        rgb   (byte-array (* 3 npx))
        err   (double-array npx)
        smp   (int-array npx)
        cnt   (long-array 2)
        ft    (double-array (* 8 npx))
        fcnt  (long-array 2)
        flin  (double-array (* 3 npx))
        frgb  (byte-array (* 3 npx))
        ferr  (double-array npx)
        ret   (int-array 1)
        act   (int-array 1)
        tot   (int-array 1)
        pxs   (long-array 1)
        head  (or first-round chunk)]
    (check (call-int "rtmi_init" (int device) (int 0) ctx))
    (try
      (let [scn (create-scene! (.getValue ctx) f)]
        (try
          (check (call-int "rtmi_render_features" scn (int nx) (int ny) (int feature-samples) (long seed) (int precision)
                           (int 0) (int 0) (int nx) (int ny) ft fcnt))
          (loop [k 0]
            (let [n (min (if (zero? k) head chunk) (- ns k))]
              (check (call-int "rtmi_render_adaptive" scn (int nx) (int ny) (int k) (int n) (double 0.0) (int depth) (long seed) (int precision)
                               (int 0) (int 0) (int nx) (int ny) lin rgb err smp cnt))
              (check (call-int "rtmi_denoise" (.getValue ctx) (int nx) (int ny) lin err ft (int iterations) (double sigma-c) (double sigma-n)
                               (double sigma-a) (double sigma-d) flin frgb ferr))
              (check (call-int "rtmi_adaptive_retire" (.getValue ctx) (int nx) (int ny) ferr (double eps) ret))
              (check (call-int "rtmi_adaptive_status" (.getValue ctx) act tot pxs))
              (let [k' (+ k n)
                    m  {:samples k' :rgb8 rgb :linear lin :stderr err :pixel-samples smp :total-rays (aget cnt 0) :total-pixels (aget cnt 1)
                        :active-tiles (aget act 0) :total-tiles (aget tot 0) :denoised {:linear flin :rgb8 frgb :stderr ferr}}]
                (if (and (not= :stop (on-round m)) (< k' ns) (pos? (aget act 0)))
                  (recur k')
                  m))))
          (finally (call-int "rtmi_scene_destroy" scn))))
      (finally (call-int "rtmi_shutdown" (.getValue ctx))))))

(defn render-multi
  "The same on every GPU in `devices` from this one JVM (rtmi_render_multi): one context per device, the scene created on
  the first (Perlin tables, ImageMap pixels and media calls included) and cloned onto the others (rtmi_scene_clone), the 8x8
  tiles of the frame dealt round-robin, ONE ncclGather inside the library, assembled on the first device.  Returns what
  `render` returns; :total-rays is the sum over the devices.  The image is bit-identical to `render`'s."
  [scene nx ny ns & {:keys [depth seed devices precision] :or {depth 50 seed 0x5eed0002 devices [0] precision 0}}]
  (let [f     (flatten-scene scene)
        npx   (* nx ny)
        lin   (double-array (* 3 npx))
        rgb   (byte-array (* 3 npx))
        cnt   (long-array 2)
        ctxs  (mapv (fn [d] (let [ctx (PointerByReference.)] (check (call-int "rtmi_init" (int d) (int 0) ctx)) (.getValue ctx))) devices)]
    (try
      (let [scn0   (create-scene! (first ctxs) f)
            clones (mapv (fn [c] (let [scn (PointerByReference.)] (check (call-int "rtmi_scene_clone" scn0 c scn)) (.getValue scn)))
                         (rest ctxs))
            scenes (into [scn0] clones)
            handles (into-array com.sun.jna.Pointer scenes)]
        (try
          (check (call-int "rtmi_render_multi" (int (count scenes)) handles
                           (int nx) (int ny) (int ns) (int depth) (long seed) (int precision) lin rgb cnt))
          {:rgb8 rgb :linear lin :total-rays (aget cnt 0) :total-pixels (aget cnt 1)}
          (finally (doseq [s scenes] (call-int "rtmi_scene_destroy" s)))))
      (finally (doseq [c ctxs] (call-int "rtmi_shutdown" c))))))

(defn render-multi-adaptive
  "render-adaptive on every GPU in `devices` from this one JVM (rtmi_render_multi_adaptive): contexts and scene replicas as in render-multi, the
  8x8 tiles of the ONE frame dealt round-robin, every replica refining its own tiles, one gather of the tile records per round, assembled on the
  first device.  Rounds, on-round, m and the return value are render-adaptive's (:active-tiles and :total-tiles summed over the devices);
  :retire false gives the progressive rule (no tile retires, eps is not read).  Every array is bit-identical to render-adaptive's on one GPU."
  [scene nx ny ns chunk eps on-round & {:keys [first-round retire depth seed devices precision]
                                        :or {retire true depth 50 seed 0x5eed0002 devices [0] precision 0}}]
  (let [f     (flatten-scene scene)
        npx   (* nx ny)
        lin   (double-array (* 3 npx))
        rgb   (byte-array (* 3 npx))
        err   (double-array npx)
        smp   (int-array npx)
        cnt   (long-array 2)
        act   (int-array 1)
        tot   (int-array 1)
        pxs   (long-array 1)
        head  (or first-round chunk)
        ctxs  (mapv (fn [d] (let [ctx (PointerByReference.)] (check (call-int "rtmi_init" (int d) (int 0) ctx)) (.getValue ctx))) devices)]
    (try
      (let [scn0   (create-scene! (first ctxs) f)
            clones (mapv (fn [c] (let [scn (PointerByReference.)] (check (call-int "rtmi_scene_clone" scn0 c scn)) (.getValue scn)))
                         (rest ctxs))
            scenes (into [scn0] clones)
            handles (into-array com.sun.jna.Pointer scenes)
            status (fn [] (reduce (fn [[a t] c] (check (call-int "rtmi_adaptive_status" c act tot pxs)) [(+ a (aget act 0)) (+ t (aget tot 0))])
                                  [0 0] ctxs))]
        (try
          (loop [k 0]
            (let [n (min (if (zero? k) head chunk) (- ns k))]
              (check (call-int "rtmi_render_multi_adaptive" (int (count scenes)) handles (int nx) (int ny) (int k) (int n) (int (if retire 1 0))
                               (double eps) (int depth) (long seed) (int precision) lin rgb err smp cnt))
              (let [k'              (+ k n)
                    [active total]  (status)
                    m  {:samples k' :rgb8 rgb :linear lin :stderr err :pixel-samples smp :total-rays (aget cnt 0) :total-pixels (aget cnt 1)
                        :active-tiles active :total-tiles total}]
                (if (and (not= :stop (on-round m)) (< k' ns) (pos? active))
                  (recur k')
                  m))))
          (finally (doseq [s scenes] (call-int "rtmi_scene_destroy" s)))))
      (finally (doseq [c ctxs] (call-int "rtmi_shutdown" c))))))

(defn render-multi-lit
  "render-lit (estimator 0 plain, 1 the NEE rule, 2 the MIS rule; :volume true the volume rule; estimator 3 the proposal rule of render-lit-ris) on
  every GPU in `devices` from this one JVM (rtmi_multi_lit_render): contexts and scene replicas as in render-multi, the 8x8 tiles of the ONE frame
  dealt round-robin, `chunk` samples per call (default: one call), one gather of the tile records per call, assembled on the first device.
  Returns {:linear :rgb8 :stderr :pixel-samples :segments :total-rays :shadow-rays :shadow-rays-occluded (summed over the calls and devices)}.
  Every array is bit-identical to the single-device call's."
  [scene nx ny ns lights & {:keys [chunk estimator light-choice volume seed depth devices precision]
                            :or {estimator 2 light-choice 0 volume false seed 0x5eed0002 depth 50 devices [0] precision 0}}]
  (let [f     (flatten-scene scene)
        fh    (long-array 1)
        npx   (* nx ny)
        lp    (int-array (if (seq lights) lights [0]))
        nl    (count lights)
        lin   (double-array (* 3 npx))
        rgb   (byte-array (* 3 npx))
        err   (double-array npx)
        smp   (int-array npx)
        cnt   (long-array 4)
        sums  (long-array 4)
        step  (or chunk ns)
        ctxs  (mapv (fn [d] (let [ctx (PointerByReference.)] (check (call-int "rtmi_init" (int d) (int 0) ctx)) (.getValue ctx))) devices)]
    (try
      (let [scn0   (create-scene! (first ctxs) f)
            clones (mapv (fn [c] (let [scn (PointerByReference.)] (check (call-int "rtmi_scene_clone" scn0 c scn)) (.getValue scn)))
                         (rest ctxs))
            scenes (into [scn0] clones)
            handles (into-array com.sun.jna.Pointer scenes)]
        (try
          (check (call-int "rtmi_multi_lit_create" (int (count scenes)) handles (int nx) (int ny) fh))
          (try
            (loop [k 0]
              (let [n (min step (- ns k))]
                (check (call-int "rtmi_multi_lit_render" (long (aget fh 0)) (int precision) (int n) (int depth) (long seed) (int estimator) (int nl) lp
                                 (int light-choice) (int (if volume 1 0)) lin rgb err smp cnt))
                (dotimes [i 4] (aset sums i (+ (aget sums i) (aget cnt i))))
                (if (< (+ k n) ns)
                  (recur (+ k n))
                  {:linear lin :rgb8 rgb :stderr err :pixel-samples smp :segments (aget sums 0) :total-rays (aget sums 1)
                   :shadow-rays (aget sums 2) :shadow-rays-occluded (aget sums 3)})))
            (finally (call-int "rtmi_multi_lit_destroy" (long (aget fh 0)))))
          (finally (doseq [s scenes] (call-int "rtmi_scene_destroy" s)))))
      (finally (doseq [c ctxs] (call-int "rtmi_shutdown" c))))))

(defn render-multi-lit-adaptive
  "render-lit-adaptive on every GPU in `devices` from this one JVM: rounds of rtmi_multi_lit_render (`first-round` samples, default `chunk`, then
  `chunk`) each followed by rtmi_multi_lit_retire by the assembled frame's standard error -- on a replica's own tiles that is the replica's own
  plane, bit for bit; a NULL map would spare the upload of 8 bytes per pixel per round, but every array argument of this file is a typed primitive
  array, which is what its conformance reader checks call site by call site -- until no tile is listed or `ns` is reached.  After each round (on-round m), m = {:samples k :linear :rgb8 :stderr
  :pixel-samples :active-tiles :total-tiles :segments :total-rays :shadow-rays :shadow-rays-occluded (summed over the rounds and devices)}; on-round
  returning :stop ends the render early.  Every array and every round's list are bit-identical to render-lit-adaptive's on one GPU.  Returns the last m."
  [scene nx ny ns chunk eps lights on-round & {:keys [first-round estimator light-choice volume seed depth devices precision]
                                               :or {estimator 2 light-choice 0 volume false seed 0x5eed0002 depth 50 devices [0] precision 0}}]
  (let [f     (flatten-scene scene)
        fh    (long-array 1)
        npx   (* nx ny)
        total (* (quot (+ nx 7) 8) (quot (+ ny 7) 8))
        lp    (int-array (if (seq lights) lights [0]))
        nl    (count lights)
        lin   (double-array (* 3 npx))
        rgb   (byte-array (* 3 npx))
        err   (double-array npx)
        smp   (int-array npx)
        cnt   (long-array 4)
        sums  (long-array 4)
        left  (int-array 1)
        held  (int-array 1)
        head  (or first-round chunk)
        ctxs  (mapv (fn [d] (let [ctx (PointerByReference.)] (check (call-int "rtmi_init" (int d) (int 0) ctx)) (.getValue ctx))) devices)]
    (try
      (let [scn0   (create-scene! (first ctxs) f)
            clones (mapv (fn [c] (let [scn (PointerByReference.)] (check (call-int "rtmi_scene_clone" scn0 c scn)) (.getValue scn)))
                         (rest ctxs))
            scenes (into [scn0] clones)
            handles (into-array com.sun.jna.Pointer scenes)]
        (try
          (check (call-int "rtmi_multi_lit_create" (int (count scenes)) handles (int nx) (int ny) fh))
          (try
            (loop []
              (check (call-int "rtmi_multi_lit_status" (long (aget fh 0)) held left))
              (let [k (aget held 0)
                    n (min (if (zero? k) head chunk) (- ns k))]
                (check (call-int "rtmi_multi_lit_render" (long (aget fh 0)) (int precision) (int n) (int depth) (long seed) (int estimator) (int nl) lp
                                 (int light-choice) (int (if volume 1 0)) lin rgb err smp cnt))
                (check (call-int "rtmi_multi_lit_retire" (long (aget fh 0)) err (double eps) left))
                (dotimes [i 4] (aset sums i (+ (aget sums i) (aget cnt i))))
                (let [k' (+ k n)
                      m  {:samples k' :linear lin :rgb8 rgb :stderr err :pixel-samples smp :active-tiles (aget left 0) :total-tiles total
                          :segments (aget sums 0) :total-rays (aget sums 1) :shadow-rays (aget sums 2) :shadow-rays-occluded (aget sums 3)}]
                  (if (and (not= :stop (on-round m)) (< k' ns) (pos? (aget left 0)))
                    (recur)
                    m))))
            (finally (call-int "rtmi_multi_lit_destroy" (long (aget fh 0)))))
          (finally (doseq [s scenes] (call-int "rtmi_scene_destroy" s)))))
      (finally (doseq [c ctxs] (call-int "rtmi_shutdown" c))))))

(defn save-ppm
  "imagez `save` (core.clj:112) has no PPM writer; binary P6 written here"
  [filename ^bytes rgb8 nx ny]
  (with-open [o (java.io.FileOutputStream. ^String filename)]
    (.write o (.getBytes (format "P6\n%d %d\n255\n" nx ny)))
    (.write o rgb8)))

(defn save-image
  "what core.clj:104-106,112 does with the pixels: an imagez image saved by extension (PNG by default, core.clj:76).
  rgb8 is row-major with row 0 = top, so no flip is needed here."
  [filename ^bytes rgb8 nx ny]
  (let [image (new-image nx ny)]
    (doseq [j (range ny) i (range nx)]
      (let [o (* 3 (+ i (* j nx)))]
        (set-pixel image i j (rgb-from-components (bit-and 0xff (aget rgb8 o))
                                                  (bit-and 0xff (aget rgb8 (+ o 1)))
                                                  (bit-and 0xff (aget rgb8 (+ o 2)))))))
    (save image filename)))

(defn -main
  "lein run name nx ny ns -- same positional arguments as raytrace-clj.core/-main (core.clj:73-80);
  renders the cover scene (the commented-out line core.clj:89)."
  [& [name ix iy is which]]
  (let [tstart   (System/currentTimeMillis)
        filename (or name "render.png")
        nx (if ix (Integer/parseUnsignedInt ix) 200)
        ny (if iy (Integer/parseUnsignedInt iy) 100)
        nr (if is (Integer/parseUnsignedInt is) 100)
        sc (if (= which "final")
             (scene/make-final nx ny)                 ; core.clj:90 (needs earth.png in the working directory)
             (scene/make-random-scene nx ny 11 true)) ; core.clj:89
        {:keys [rgb8 total-rays total-pixels]} (render sc nx ny nr)
        elapsed (/ (- (System/currentTimeMillis) tstart) 1000.0)]
    (println (format "%.2fs, %d%%, ETA %.2fs" elapsed 100 0.0))      ; display.clj:20-24
    (println "total-rays" total-rays "total-pixels" total-pixels)    ; metrics.clj:8-9
    (if (.endsWith (.toLowerCase ^String filename) ".ppm")
      (save-ppm filename rgb8 nx ny)
      (save-image filename rgb8 nx ny))
    (println "wrote" filename)))                                     ; core.clj:113
